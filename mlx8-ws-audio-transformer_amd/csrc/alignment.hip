// Token-level timestamps of Whisper's generate (HF 5.15 `WhisperGenerationMixin._extract_token_timestamps`,
// transformers/models/whisper/generation_whisper.py:241-381), gfx950: the cross-attention probabilities of the alignment heads,
// the z-score / median-filter / head-mean matrix, and dynamic time warping over it.  Three launches per decode call, no atomics,
// bit-reproducible.
//
//  * align_weights_kernel: the decoder's cross-attention runs flash-style (decoder_ops.hip small_attn_fwd_kernel) and never holds a
//    probability row, so the rows the alignment needs are recomputed from the query rows the decoding steps kept: one workgroup per
//    (clip, selected head, 8 token rows), lane j forms the scores of key j against the 8 queries exactly as the decoder does (q scaled
//    by 0.125 in LDS, the key row in registers, the same fp32 summation order), the 8 x S scores stay in LDS, and the softmax runs over
//    ALL S encoder positions before the store crops to the frames asked for.
//  * align_matrix_kernel: per (clip, head, frame) the z-score over the token rows, a width-w median along frames with reflect padding and
//    the mean over heads.  A workgroup owns 64 frames plus a w / 2 halo, so the per-column statistics need no second launch.
//  * dtw_kernel: one workgroup per clip, thread i owns token row i, anti-diagonal sweep.  cost[i][j] = float(double(m) + double(c)) with
//    HF's tie rule, so the costs are the reference's bit for bit; the 2-bit trace goes to a diagonal-major byte workspace (coalesced
//    stores); one lane walks the trace back.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ probabilities of the alignment heads
constexpr int kAwRows = 8;          // token rows per workgroup
constexpr int kAwMaxS = 1536;       // encoder positions whose scores fit the workgroup's LDS

struct AlignW {
  const float* q; int64_t q_slot_stride, q_row_stride;     // q[slot][row][position][d]
  const float* kv; int ldkv;                               // cross_kv: row (clip S + j), keys of layer l at column 2 l d
  const int32_t* heads;                                    // [n_sel][3]: slot in q, decoder layer, head
  const int32_t* src_row;                                  // [clips][T] row of q that decoded (clip, t), or null: the clip's own row
  int rows, group, n_slots, n_layers, d, S, n_sel, clips, t0, T;
  float* out; int frames;                                  // [clips][n_sel][T][frames]
};

__global__ __launch_bounds__(256) void align_weights_kernel(AlignW a) {
  __shared__ __attribute__((aligned(16))) float qs[kAwRows][64];
  __shared__ float sc[kAwRows][kAwMaxS];
  __shared__ int kclip[kAwRows];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int hsel = blockIdx.x % a.n_sel, clip = blockIdx.x / a.n_sel;
  const int i0 = blockIdx.y * kAwRows, nq = min(kAwRows, a.T - i0);
  const int slot = min(max(a.heads[3 * hsel], 0), a.n_slots - 1);
  const int layer = min(max(a.heads[3 * hsel + 1], 0), a.n_layers - 1);
  const int head = min(max(a.heads[3 * hsel + 2], 0), a.d / 64 - 1);
  for (int t = threadIdx.x; t < kAwRows * 64; t += 256) {
    const int i = t >> 6, e = t & 63;
    float v = 0.f;
    if (i < nq) {
      int r = a.src_row ? a.src_row[(int64_t)clip * a.T + i0 + i] : clip * a.group;
      r = min(max(r, 0), a.rows - 1);
      v = a.q[slot * a.q_slot_stride + r * a.q_row_stride + (int64_t)(a.t0 + i0 + i) * a.d + 64 * head + e] * 0.125f;
      if (e == 0) kclip[i] = r / a.group;
    } else if (e == 0) {
      kclip[i] = -1;
    }
    qs[i][e] = v;
  }
  __syncthreads();
  // rows of a tile attend to their own clip's keys, except rows that beam search filled with row 0 of the batch (clip 0): one pass per
  // distinct clip among the tile's rows
  for (int first = 0; first < nq; ++first) {
    const int kc = kclip[first];
    bool seen = false;
    for (int p = 0; p < first; ++p) seen |= kclip[p] == kc;
    if (seen) continue;
    const float* kp = a.kv + (int64_t)kc * a.S * a.ldkv + 2 * layer * a.d + 64 * head;
    for (int c = wave; c * 64 < a.S; c += 4) {
      const int j = c * 64 + lane;
      const float* kr = kp + (int64_t)min(j, a.S - 1) * a.ldkv;
      float k[64];
#pragma unroll
      for (int e = 0; e < 64; e += 4) { const float4 t = *reinterpret_cast<const float4*>(kr + e); k[e] = t.x; k[e + 1] = t.y; k[e + 2] = t.z; k[e + 3] = t.w; }
#pragma unroll
      for (int i = 0; i < kAwRows; ++i) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 64; e += 4) { const float4 t = *reinterpret_cast<const float4*>(&qs[i][e]); s += t.x * k[e] + t.y * k[e + 1] + t.z * k[e + 2] + t.w * k[e + 3]; }
        if (j < a.S && kclip[i] == kc) sc[i][j] = s;
      }
    }
  }
  __syncthreads();
  for (int i = wave; i < nq; i += 4) {
    float m = -3.0e38f;
    for (int j = lane; j < a.S; j += 64) m = fmaxf(m, sc[i][j]);
    m = wave_max(m);
    float l = 0.f;
    for (int j = lane; j < a.S; j += 64) { const float e = __expf(sc[i][j] - m); sc[i][j] = e; l += e; }
    l = wave_sum(l);
    float* o = a.out + (((int64_t)clip * a.n_sel + hsel) * a.T + i0 + i) * a.frames;
    for (int j = lane; j < a.frames; j += 64) o[j] = sc[i][j] / l;
  }
}

// ------------------------------------------------------------------------------------------------ z-score, median filter, head mean
constexpr int kAmTile = 64;                         // output frames per workgroup
constexpr int kAmMaxWidth = 15;
constexpr int kAmCols = kAmTile + kAmMaxWidth - 1;  // the tile and its halo
constexpr int kAmStatCols = 80;                     // threads per token-row group of the statistics pass
static_assert(kAmCols <= kAmStatCols && 3 * kAmStatCols <= 256, "the staged tile must fit one statistics group");
constexpr int kAmMaxHeads = 32;

struct AlignM {
  const float* w;            // [clips][n_sel][T][frames]
  const int32_t* nf;         // frames of each clip, or null: `frames`
  int clips, n_sel, T, frames, width;
  float* out;                // [clips][T][frames]
};

// median of W values (W odd): odd-even transposition network in registers; NaN orders last, as torch.sort does
template <int W>
__device__ __forceinline__ float median_of(const float* z) {
  float v[W];
#pragma unroll
  for (int k = 0; k < W; ++k) v[k] = z[k];
#pragma unroll
  for (int r = 0; r < W; ++r) {
#pragma unroll
    for (int k = r & 1; k + 1 < W; k += 2) {
      const float x = v[k], y = v[k + 1];
      const bool swap = x > y || (x != x && y == y);
      v[k] = swap ? y : x;
      v[k + 1] = swap ? x : y;
    }
  }
  return v[W / 2];
}

__device__ __forceinline__ float median_width(const float* z, int width) {
  switch (width) {
    case 1: return z[0];
    case 3: return median_of<3>(z);
    case 5: return median_of<5>(z);
    case 7: return median_of<7>(z);
    case 9: return median_of<9>(z);
    case 11: return median_of<11>(z);
    case 13: return median_of<13>(z);
    default: return median_of<15>(z);
  }
}

__global__ __launch_bounds__(256) void align_matrix_kernel(AlignM a) {
  __shared__ float mean_s[kAmMaxHeads][kAmStatCols], std_s[kAmMaxHeads][kAmStatCols];
  __shared__ double part[3][kAmStatCols];
  __shared__ float zs[4][kAmStatCols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int clip = blockIdx.y, f0 = blockIdx.x * kAmTile;
  const int F = min(max(a.nf ? a.nf[clip] : a.frames, 0), a.frames);
  float* out = a.out + (int64_t)clip * a.T * a.frames;
  if (f0 >= F) {                                                      // beyond the clip's frames: defined, never read by the DTW
    for (int t = wave; t < a.T; t += 4)
      if (f0 + lane < a.frames) out[(int64_t)t * a.frames + f0 + lane] = 0.f;
    return;
  }
  const int pad = F <= a.width / 2 ? 0 : a.width / 2;                 // HF returns the input unfiltered when frames <= width / 2
  const int weff = 2 * pad + 1;
  const int nout = min(kAmTile, F - f0), ncol = nout + 2 * pad;
  // column c of the staged tile is frame g = f0 - pad + c of the reflect-padded row (pad < F, so one reflection lands inside)
  auto source = [&](int c) { const int g = f0 - pad + c; return g < 0 ? -g : (g >= F ? 2 * (F - 1) - g : g); };
  const int sc = threadIdx.x % kAmStatCols, sg = threadIdx.x / kAmStatCols;      // statistics: column, token-row group (3 groups)
  const bool stat = sg < 3 && sc < ncol;
  const int ssrc = stat ? source(sc) : 0;
  for (int h = 0; h < a.n_sel; ++h) {
    const float* w = a.w + ((int64_t)clip * a.n_sel + h) * a.T * a.frames;
    double s = 0.0;
    if (stat) for (int t = sg; t < a.T; t += 3) s += (double)w[(int64_t)t * a.frames + ssrc];
    if (stat) part[sg][sc] = s;
    __syncthreads();
    if (stat && sg == 0) mean_s[h][sc] = (float)((part[0][sc] + part[1][sc] + part[2][sc]) / (double)a.T);
    __syncthreads();
    s = 0.0;
    if (stat) {
      const float mu = mean_s[h][sc];
      for (int t = sg; t < a.T; t += 3) { const float dlt = w[(int64_t)t * a.frames + ssrc] - mu; s += (double)dlt * (double)dlt; }
      part[sg][sc] = s;
    }
    __syncthreads();
    if (stat && sg == 0) std_s[h][sc] = (float)sqrt((part[0][sc] + part[1][sc] + part[2][sc]) / (double)a.T);
    __syncthreads();
  }
  const float inv_heads = 1.0f / (float)a.n_sel;
  for (int tb = 0; tb < a.T; tb += 4) {
    const int t = tb + wave;
    const bool row = t < a.T;
    float acc = 0.f;
    for (int h = 0; h < a.n_sel; ++h) {
      if (row) {
        const float* w = a.w + (((int64_t)clip * a.n_sel + h) * a.T + t) * a.frames;
        for (int c = lane; c < ncol; c += 64) zs[wave][c] = (w[source(c)] - mean_s[h][c]) / std_s[h][c];
      }
      __syncthreads();
      if (row && lane < nout) acc += median_width(&zs[wave][lane], weff);
      __syncthreads();
    }
    if (row) {
      if (lane < nout) out[(int64_t)t * a.frames + f0 + lane] = acc * inv_heads;
      else if (f0 + lane < a.frames) out[(int64_t)t * a.frames + f0 + lane] = 0.f;
    }
  }
}

// ------------------------------------------------------------------------------------------------ dynamic time warping
constexpr int kDtwMaxT = 448;

struct Dtw {
  const float* m;            // [clips][T][frames]
  const int32_t* nf;         // frames of each clip, or null: `frames`
  int T, frames, negate, cap;
  uint8_t* trace;            // per clip (T + frames) x T bytes, diagonal-major: the cell (i, j) at (i + j) T + i
  int32_t *jump, *text_idx, *time_idx, *path_start;
};

__global__ __launch_bounds__(kDtwMaxT) void dtw_kernel(Dtw a) {
  __shared__ float edge[2][8];
  const int clip = blockIdx.x, i = threadIdx.x, lane = i & 63, wave = i >> 6;
  const int T = a.T;
  const int F = min(max(a.nf ? a.nf[clip] : a.frames, 0), a.frames);
  const float inf = __builtin_inff();
  const float* row = a.m + ((int64_t)clip * T + min(i, T - 1)) * a.frames;
  uint8_t* tr = a.trace + (int64_t)clip * (T + a.frames) * T;
  if (i < 16) edge[i >> 3][i & 7] = inf;
  __syncthreads();
  // HF's cost array has a row 0 and a column 0: cost[0][0] = 0, every other cell of them inf.  Thread i holds cost[i + 1][.]; `cur` is its
  // newest cell, `nb` the upper neighbour's newest (cost[i][j + 1]) and `prev_nb` the one before (cost[i][j]).
  float cur = inf, prev_nb = i == 0 ? 0.f : inf;
  float mnext = (i == 0 && F > 0) ? row[0] : 0.f;
  const int nsteps = F > 0 ? T + F - 1 : 0;
  for (int s = 0; s < nsteps; ++s) {
    float nb = __shfl_up(cur, 1);
    if (lane == 0) nb = wave == 0 ? inf : edge[(s + 1) & 1][wave - 1];
    const int j = s - i;
    const float mv = mnext;
    if (i < T && j + 1 >= 0 && j + 1 < F) mnext = row[j + 1];
    if (i < T && j >= 0 && j < F) {
      const float c0 = prev_nb, c1 = nb, c2 = cur;
      float c; int t;
      if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
      else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
      else { c = c2; t = 2; }
      cur = (float)((double)(a.negate ? -mv : mv) + (double)c);
      tr[(int64_t)s * T + i] = (uint8_t)t;
    }
    prev_nb = nb;
    if (lane == 63) edge[s & 1][wave] = cur;
    __syncthreads();
  }
  __threadfence();
  __syncthreads();
  if (i != 0) return;
  // backtrace (HF: trace[0, :] = 2, trace[:, 0] = 1), written from the end of the path arrays backwards
  int32_t* tx = a.text_idx + (int64_t)clip * a.cap;
  int32_t* tm = a.time_idx + (int64_t)clip * a.cap;
  int32_t* jump = a.jump + (int64_t)clip * T;
  int ii = T, jj = F, k = a.cap - 1;
  if (F <= 0) { for (int t = 0; t < T; ++t) jump[t] = 0; a.path_start[clip] = a.cap; return; }
  while ((ii > 0 || jj > 0) && k >= 0) {
    tx[k] = ii - 1;
    tm[k] = jj - 1;
    if (ii > 0) jump[ii - 1] = jj - 1;                    // the last write to a row is the path's first cell of that row
    const int t = ii == 0 ? 2 : (jj == 0 ? 1 : tr[(int64_t)(ii + jj - 2) * T + ii - 1]);
    if (t == 0) { --ii; --jj; } else if (t == 1) { --ii; } else { --jj; }
    --k;
  }
  a.path_start[clip] = k + 1;
}

}  // namespace

extern "C" int awt_op_alignment_weights(awt_ctx* c, const float* q, int n_slots, int rows, int Tmax, int d, int group, const float* cross_kv,
                                        int n_layers, int S, const int32_t* heads, int n_sel, const int32_t* src_row, int clips, int t0, int T,
                                        float* out, int frames, void* stream) {
  AWT_REQUIRE(c && q && cross_kv && heads && out, AWT_ERR_INVALID, "op_alignment_weights: null argument");
  AWT_REQUIRE(d >= 64 && d % 64 == 0, AWT_ERR_INVALID, "op_alignment_weights: d must be a positive multiple of 64 (head_dim 64)");
  AWT_REQUIRE(S >= 1 && S <= kAwMaxS, AWT_ERR_INVALID, "op_alignment_weights: need 1 <= S <= " + std::to_string(kAwMaxS) + " encoder positions");
  AWT_REQUIRE(frames >= 1 && frames <= S, AWT_ERR_INVALID, "op_alignment_weights: need 1 <= frames <= S");
  AWT_REQUIRE(n_slots >= 1 && n_layers >= 1 && n_sel >= 1 && clips >= 1 && rows >= 1 && group >= 1 && rows % group == 0, AWT_ERR_INVALID,
              "op_alignment_weights: need positive counts and rows a multiple of group");
  AWT_REQUIRE(src_row || rows == clips * group, AWT_ERR_INVALID, "op_alignment_weights: without src_row, rows must be clips x group");
  AWT_REQUIRE(T >= 1 && t0 >= 0 && t0 + T <= Tmax, AWT_ERR_INVALID, "op_alignment_weights: need T >= 1 and t0 + T <= Tmax");
  AWT_REQUIRE((((uintptr_t)cross_kv) & 15) == 0, AWT_ERR_INVALID, "op_alignment_weights: cross_kv must be 16-byte aligned (float4 loads)");
  AlignW a{};
  a.q = q; a.q_slot_stride = (int64_t)rows * Tmax * d; a.q_row_stride = (int64_t)Tmax * d;
  a.kv = cross_kv; a.ldkv = 2 * n_layers * d; a.heads = heads; a.src_row = src_row;
  a.rows = rows; a.group = group; a.n_slots = n_slots; a.n_layers = n_layers; a.d = d; a.S = S; a.n_sel = n_sel; a.clips = clips; a.t0 = t0; a.T = T;
  a.out = out; a.frames = frames;
  hipLaunchKernelGGL(align_weights_kernel, dim3(clips * n_sel, (T + kAwRows - 1) / kAwRows), dim3(256), 0, (hipStream_t)stream, a);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" int awt_op_alignment_matrix(awt_ctx* c, const float* weights, int clips, int n_sel, int T, int frames, const int32_t* num_frames, int width,
                                       float* out, void* stream) {
  AWT_REQUIRE(c && weights && out, AWT_ERR_INVALID, "op_alignment_matrix: null argument");
  AWT_REQUIRE(clips >= 1 && T >= 1 && frames >= 1, AWT_ERR_INVALID, "op_alignment_matrix: need clips, T, frames >= 1");
  AWT_REQUIRE(n_sel >= 1 && n_sel <= kAmMaxHeads, AWT_ERR_INVALID, "op_alignment_matrix: need 1 <= heads <= " + std::to_string(kAmMaxHeads));
  AWT_REQUIRE(width >= 1 && width <= kAmMaxWidth && width % 2 == 1, AWT_ERR_VALUE,
              "median_filter_width must be odd and between 1 and " + std::to_string(kAmMaxWidth) + ", got " + std::to_string(width));
  AlignM a{weights, num_frames, clips, n_sel, T, frames, width, out};
  hipLaunchKernelGGL(align_matrix_kernel, dim3((frames + kAmTile - 1) / kAmTile, clips), dim3(256), 0, (hipStream_t)stream, a);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" size_t awt_dtw_workspace_bytes(int clips, int T, int frames) {
  if (clips <= 0 || T <= 0 || frames <= 0) return 0;
  return (size_t)clips * ((size_t)T + frames) * T + 256;
}

extern "C" int awt_op_dtw(awt_ctx* c, const float* matrix, int clips, int T, int frames, const int32_t* num_frames, int negate, int32_t* jump_frame,
                          int32_t* text_idx, int32_t* time_idx, int32_t* path_start, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && matrix && jump_frame && text_idx && time_idx && path_start && workspace, AWT_ERR_INVALID, "op_dtw: null argument");
  AWT_REQUIRE(clips >= 1 && frames >= 1, AWT_ERR_INVALID, "op_dtw: need clips, frames >= 1");
  AWT_REQUIRE(T >= 1 && T <= kDtwMaxT, AWT_ERR_INVALID, "op_dtw: need 1 <= T <= " + std::to_string(kDtwMaxT) + " token rows (one thread each)");
  const size_t need = awt_dtw_workspace_bytes(clips, T, frames);
  AWT_REQUIRE(ws_bytes >= need, AWT_ERR_INVALID, "op_dtw: workspace too small (" + std::to_string(ws_bytes) + " < " + std::to_string(need) + " bytes)");
  Dtw a{};
  a.m = matrix; a.nf = num_frames; a.T = T; a.frames = frames; a.negate = negate; a.cap = T + frames;
  a.trace = static_cast<uint8_t*>(workspace); a.jump = jump_frame; a.text_idx = text_idx; a.time_idx = time_idx; a.path_start = path_start;
  hipLaunchKernelGGL(dtw_kernel, dim3(clips), dim3((T + 63) / 64 * 64), 0, (hipStream_t)stream, a);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}
