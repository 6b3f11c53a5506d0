// Operators of the 1-D CNN classifier (cnn_classifier.py), gfx950: Conv1d(k = 3, padding = 1) as one row-mapped GEMM, and
// training-mode BatchNorm1d + ReLU + pooling with their backward.
//
// Activations are channels-last fp32 rows [B T, C] -- what the GEMM reads and writes -- so a channel is a COLUMN and BatchNorm's statistics are
// column statistics over M = B T rows.  Everything except the conv is HBM-bound; the design unit is a pass over the [M, C] tensor:
//   forward   conv (GEMM)  ->  stats: 1 read of x  ->  bn_relu_pool: 1 read of x, 1 write of the pooled y (half the rows, or one row per clip)
//   backward  reduce: 1 read of x (+ the pooled dy)  ->  apply: 1 read of x (+ dy), 1 write of dx  ->  conv gradients (GEMMs)
// The normalised tensor, the ReLU mask and the arg-max of the pooling are never stored: both backward kernels recompute them from the saved
// pre-BN x with the forward's own arithmetic (bn_act below), which is cheaper than a second [M, C] tensor through HBM.
//
// Thread layout of every row kernel: a workgroup is 32 column groups (one float4 = 4 channels per lane: 32 lanes cover 512 contiguous bytes of a
// row) x 8 row lanes, and owns 128 channels of one SLAB of 64 row units; row lane y walks units y, y + 8, ...  Reductions are deterministic: the
// 8 row lanes of a slab are merged in lane order through LDS, the slabs in slab order by a second, tiny launch.  No atomics, no hidden
// synchronisation; every launch goes to the caller's stream.
#include <initializer_list>

#include "common.h"

namespace {

constexpr int kCols = 32;                 // column groups (float4) per workgroup: 128 channels
constexpr int kLanes = 8;                 // row lanes per workgroup
constexpr int kPerLane = 8;               // row units per row lane
constexpr int kSlab = kLanes * kPerLane;  // row units per workgroup

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float4 max4(const float4 a, const float4 b) { return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)); }

// ------------------------------------------------------------------------------------------------ batch statistics
// Merge of two (count, mean, sum of squared deviations) triples (Chan et al.): exact for equal means, and free of the cancellation of
// E[x^2] - E[x]^2.  na = 0 (the empty start) gives (nb, mb, Sb).
__device__ __forceinline__ void chan_merge(float& na, float4& ma, float4& Sa, float nb, const float4 mb, const float4 Sb) {
  const float n = na + nb, f = nb / n, g = na * f;
  const float4 d = mb - ma;
  ma = ma + d * f;
  Sa = Sa + Sb + d * d * g;
  na = n;
}

// partial[slab][0][C] = mean, partial[slab][1][C] = sum of squared deviations of the slab's rows.  A row lane holds its <= 8 rows in registers
// and makes two passes over them: the mean as first row + mean of the differences to it (exact for a constant column), then the deviations.
__global__ __launch_bounds__(256) void bn_stats_slab_kernel(const float* __restrict__ x, int M, int C, float* __restrict__ partial) {
  __shared__ float4 sm[kLanes][kCols], sS[kLanes][kCols];
  const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
  const int col = (blockIdx.x * kCols + tx) * 4;
  const bool col_ok = col < C;
  const int r0 = blockIdx.y * kSlab, rows = min(kSlab, M - r0);
  const int n = rows > ty ? (rows - ty + kLanes - 1) / kLanes : 0;       // rows of this lane: r0 + ty + 8 j, j < n
  float4 v[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) v[j] = (j < n && col_ok) ? ld4(x + (int64_t)(r0 + ty + kLanes * j) * C + col) : f4(0.f);
  float4 d = f4(0.f);
#pragma unroll
  for (int j = 1; j < kPerLane; ++j) if (j < n) d = d + (v[j] - v[0]);
  const float4 mean = n > 0 ? v[0] + d * (1.0f / (float)n) : f4(0.f);
  float4 S = f4(0.f);
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) if (j < n) { const float4 e = v[j] - mean; S = S + e * e; }
  sm[ty][tx] = mean; sS[ty][tx] = S;
  __syncthreads();
  if (ty != 0 || !col_ok) return;
  float na = 0.f; float4 ma = f4(0.f), Sa = f4(0.f);
#pragma unroll
  for (int y = 0; y < kLanes; ++y) {
    const int ny = rows > y ? (rows - y + kLanes - 1) / kLanes : 0;
    if (ny > 0) chan_merge(na, ma, Sa, (float)ny, sm[y][tx], sS[y][tx]);
  }
  float* p = partial + (int64_t)blockIdx.y * 2 * C + col;
  st4(p, ma); st4(p + C, Sa);
}
// the slabs in ascending order; var = S / M (biased, what BatchNorm normalises with)
__global__ __launch_bounds__(256) void bn_stats_merge_kernel(const float* __restrict__ partial, int nslab, int M, int C, float* mean, float* var) {
  const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (col >= C) return;
  float na = 0.f; float4 ma = f4(0.f), Sa = f4(0.f);
  for (int i = 0; i < nslab; ++i) {
    const float* p = partial + (int64_t)i * 2 * C + col;
    chan_merge(na, ma, Sa, (float)min(kSlab, M - i * kSlab), ld4(p), ld4(p + C));
  }
  st4(mean + col, ma); st4(var + col, Sa * (1.0f / (float)M));
}

// ------------------------------------------------------------------------------------------------ BatchNorm + ReLU + pooling
// The four channels' affine map, loaded once per thread.  xhat = (x - mean) rstd and z = xhat gamma + beta are formed by ONE function in the
// forward and in both backward kernels, so the recomputed ReLU mask and pooling winner are those of the forward bit for bit.
struct BnCoef { float4 mean, rstd, gamma, beta; };
__device__ __forceinline__ BnCoef bn_coef(const float* mean, const float* var, const float* gamma, const float* beta, float eps, int col) {
  BnCoef k;
  const float4 v = ld4(var + col);
  k.mean = ld4(mean + col); k.gamma = ld4(gamma + col); k.beta = ld4(beta + col);
  k.rstd = make_float4(1.0f / sqrtf(v.x + eps), 1.0f / sqrtf(v.y + eps), 1.0f / sqrtf(v.z + eps), 1.0f / sqrtf(v.w + eps));
  return k;
}
__device__ __forceinline__ float4 bn_xhat(const BnCoef& k, const float4 x) { return (x - k.mean) * k.rstd; }
__device__ __forceinline__ float4 bn_act(const BnCoef& k, const float4 xh) {      // pre-ReLU BatchNorm output
  return make_float4(fmaf(xh.x, k.gamma.x, k.beta.x), fmaf(xh.y, k.gamma.y, k.beta.y), fmaf(xh.z, k.gamma.z, k.beta.z), fmaf(xh.w, k.gamma.w, k.beta.w));
}
// relu(NaN) = NaN as in torch (fmaxf(NaN, 0) would be 0: a channel whose statistics are NaN would come out as clean zeros)
__device__ __forceinline__ float relu1(float z) { return z <= 0.f ? 0.f : z; }
__device__ __forceinline__ float4 relu4(const float4 z) { return make_float4(relu1(z.x), relu1(z.y), relu1(z.z), relu1(z.w)); }
__device__ __forceinline__ float4 gate(const float4 z, const float4 g) {           // g where z > 0: ReLU's derivative
  return make_float4(z.x > 0.f ? g.x : 0.f, z.y > 0.f ? g.y : 0.f, z.z > 0.f ? g.z : 0.f, z.w > 0.f ? g.w : 0.f);
}
// Gradient of max_i relu(z_i) over a pooling window of W frames with respect to each z_i.  The winner is the FIRST frame holding the window's
// largest pre-ReLU value: walking the frames in order, `rem` is the part of g not yet handed out, and a frame with z_i >= max takes all of it.
// After the ReLU a tie between two DIFFERENT inputs can only be 0 = 0, where ReLU's derivative is zero whichever index is named, so the kernel
// would not have to reproduce torch's first-index tie-break; `>=` costs nothing and also covers equal positive values (a constant channel ties
// at beta).
__device__ __forceinline__ float4 take_ge(const float4 z, const float4 m, const float4 g) {
  return make_float4(z.x >= m.x ? g.x : 0.f, z.y >= m.y ? g.y : 0.f, z.z >= m.z ? g.z : 0.f, z.w >= m.w ? g.w : 0.f);
}
template <int W>
__device__ __forceinline__ void pool_grad(const float4 (&z)[W], const float4 g, float4 (&gz)[W]) {
  float4 m = z[0], rem = g;
#pragma unroll
  for (int i = 1; i < W; ++i) m = max4(m, z[i]);
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const float4 t = take_ge(z[i], m, rem);
    rem = rem - t;
    gz[i] = gate(z[i], t);
  }
}
// max over the window's W frames of the pre-ReLU BatchNorm output, then the ReLU (relu is monotone: the same value as max of the relus)
template <int W>
__device__ __forceinline__ float4 bn_relu_window_max(const BnCoef& k, const float* p, int C) {
  float4 m = bn_act(k, bn_xhat(k, ld4(p)));
#pragma unroll
  for (int i = 1; i < W; ++i) m = max4(m, bn_act(k, bn_xhat(k, ld4(p + (int64_t)i * C))));
  return relu4(m);
}

// pool = 2 / 4 (W): unit u = (clip b, pooled frame tw) reads rows b T + W tw ... + W - 1, writes row u of y [B (T / W), C]; the trailing T mod W
// frames are not read.
template <int W>
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const float* __restrict__ x, const float* mean, const float* var, const float* gamma,
                                                              const float* beta, float eps, float* __restrict__ y, int U, int T, int TW, int C) {
  const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
  const int col = (blockIdx.x * kCols + tx) * 4;
  if (col >= C) return;
  const BnCoef k = bn_coef(mean, var, gamma, beta, eps, col);
  const int u0 = blockIdx.y * kSlab + ty;
#pragma unroll 4
  for (int j = 0; j < kPerLane; ++j) {
    const int u = u0 + kLanes * j;
    if (u >= U) break;
    const int b = u / TW, tw = u - b * TW;
    st4(y + (int64_t)u * C + col, bn_relu_window_max<W>(k, x + ((int64_t)b * T + W * tw) * C + col, C));
  }
}
// pool = 0: y[b] = mean over the clip's T frames, added in frame order; unit = clip
__global__ __launch_bounds__(256) void bn_relu_avgpool_kernel(const float* __restrict__ x, const float* mean, const float* var, const float* gamma,
                                                              const float* beta, float eps, float* __restrict__ y, int B, int T, int C) {
  const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
  const int col = (blockIdx.x * kCols + tx) * 4;
  const int b = blockIdx.y * kLanes + ty;
  if (col >= C || b >= B) return;
  const BnCoef k = bn_coef(mean, var, gamma, beta, eps, col);
  const float* p = x + (int64_t)b * T * C + col;
  float4 s = f4(0.f);
  for (int t = 0; t < T; ++t, p += C) s = s + relu4(bn_act(k, bn_xhat(k, ld4(p))));
  st4(y + (int64_t)b * C + col, s * (1.0f / (float)T));
}
// MaxPool1d(4) then the mean (AWT_POOL_MAX4_MEAN): y[b] = mean over the clip's TW = T / W pooled frames, added in frame order; unit = clip.  The
// pooled tensor exists in registers only.
template <int W>
__global__ __launch_bounds__(256) void bn_relu_maxpool_mean_kernel(const float* __restrict__ x, const float* mean, const float* var, const float* gamma,
                                                                   const float* beta, float eps, float* __restrict__ y, int B, int T, int TW, int C) {
  const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
  const int col = (blockIdx.x * kCols + tx) * 4;
  const int b = blockIdx.y * kLanes + ty;
  if (col >= C || b >= B) return;
  const BnCoef k = bn_coef(mean, var, gamma, beta, eps, col);
  const float* p = x + (int64_t)b * T * C + col;
  float4 s = f4(0.f);
  for (int tw = 0; tw < TW; ++tw, p += (int64_t)W * C) s = s + bn_relu_window_max<W>(k, p, C);
  st4(y + (int64_t)b * C + col, s * (1.0f / (float)TW));
}

// Backward, launch 1: partial[slab][0][C] = sum dz, partial[slab][1][C] = sum dz xhat over the slab's units, dz the gradient at the BatchNorm
// output.  W = 2 / 4: unit = a pooled frame (W rows of x; the frames that T mod W drops have dz = 0 and add nothing) whose gradient is row u of dy,
// or with MEAN dy[clip] / TW; W = 0: unit = a row of x with dz = relu'(z) dy[clip] / T.
template <int W, bool MEAN>
__global__ __launch_bounds__(256) void bn_pool_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* mean, const float* var,
                                                                 const float* gamma, const float* beta, float eps, int U, int T, int TW, int C,
                                                                 float* __restrict__ partial) {
  __shared__ float4 s1[kLanes][kCols], s2[kLanes][kCols];
  const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
  const int col = (blockIdx.x * kCols + tx) * 4;
  const bool col_ok = col < C;
  float4 a1 = f4(0.f), a2 = f4(0.f);
  if (col_ok) {
    const BnCoef k = bn_coef(mean, var, gamma, beta, eps, col);
    const float inv_t = 1.0f / (float)T;
    const int u0 = blockIdx.y * kSlab + ty;
#pragma unroll 2
    for (int j = 0; j < kPerLane; ++j) {
      const int u = u0 + kLanes * j;
      if (u >= U) break;
      if constexpr (W > 0) {
        const int b = u / TW, tw = u - b * TW;
        const float* p = x + ((int64_t)b * T + W * tw) * C + col;
        float4 h[W], z[W], g[W];
#pragma unroll
        for (int i = 0; i < W; ++i) { h[i] = bn_xhat(k, ld4(p + (int64_t)i * C)); z[i] = bn_act(k, h[i]); }
        float4 gy;
        if constexpr (MEAN) gy = ld4(dy + (int64_t)b * C + col) * (1.0f / (float)TW); else gy = ld4(dy + (int64_t)u * C + col);
        pool_grad<W>(z, gy, g);
        if constexpr (W == 2) {
          a1 = a1 + g[0] + g[1];
          a2 = a2 + g[0] * h[0] + g[1] * h[1];
        } else {
          a1 = a1 + g[0] + g[1] + g[2] + g[3];
          a2 = a2 + g[0] * h[0] + g[1] * h[1] + g[2] * h[2] + g[3] * h[3];
        }
      } else {
        const float4 h = bn_xhat(k, ld4(x + (int64_t)u * C + col));
        const float4 g = gate(bn_act(k, h), ld4(dy + (int64_t)(u / T) * C + col) * inv_t);
        a1 = a1 + g;
        a2 = a2 + g * h;
      }
    }
  }
  s1[ty][tx] = a1; s2[ty][tx] = a2;
  __syncthreads();
  if (ty != 0 || !col_ok) return;
#pragma unroll
  for (int y = 1; y < kLanes; ++y) { a1 = a1 + s1[y][tx]; a2 = a2 + s2[y][tx]; }
  float* p = partial + (int64_t)blockIdx.y * 2 * C + col;
  st4(p, a1); st4(p + C, a2);
}
__global__ __launch_bounds__(256) void bn_pool_bwd_sum_kernel(const float* __restrict__ partial, int nslab, int C, float* dgamma, float* dbeta) {
  const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (col >= C) return;
  float4 a1 = f4(0.f), a2 = f4(0.f);
  for (int i = 0; i < nslab; ++i) {
    const float* p = partial + (int64_t)i * 2 * C + col;
    a1 = a1 + ld4(p); a2 = a2 + ld4(p + C);
  }
  st4(dbeta + col, a1); st4(dgamma + col, a2);
}
// Backward, launch 3: dx = gamma rstd (dz - dbeta / M - xhat dgamma / M) for EVERY row of x, M = B T.  W = 2 / 4: unit = (clip, window p < ceil(T / W));
// the frames of the incomplete last window have dz = 0 but still receive the two mean terms.
template <int W, bool MEAN>
__global__ __launch_bounds__(256) void bn_pool_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* mean, const float* var,
                                                                const float* gamma, const float* beta, float eps, const float* dgamma, const float* dbeta,
                                                                int U, int T, int TW, int C, float inv_m, float* __restrict__ dx) {
  const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
  const int col = (blockIdx.x * kCols + tx) * 4;
  if (col >= C) return;
  const BnCoef k = bn_coef(mean, var, gamma, beta, eps, col);
  const float4 kb = ld4(dbeta + col) * inv_m, kg = ld4(dgamma + col) * inv_m, gr = k.gamma * k.rstd;
  const float inv_t = 1.0f / (float)T;
  const int u0 = blockIdx.y * kSlab + ty;
#pragma unroll 2
  for (int j = 0; j < kPerLane; ++j) {
    const int u = u0 + kLanes * j;
    if (u >= U) break;
    if constexpr (W > 0) {
      const int Tp = (T + W - 1) / W;
      const int b = u / Tp, tp = u - b * Tp;
      const int64_t row = (int64_t)b * T + W * tp;
      if (tp < TW) {
        float4 h[W], z[W], g[W];
#pragma unroll
        for (int i = 0; i < W; ++i) { h[i] = bn_xhat(k, ld4(x + (row + i) * C + col)); z[i] = bn_act(k, h[i]); }
        float4 gy;
        if constexpr (MEAN) gy = ld4(dy + (int64_t)b * C + col) * (1.0f / (float)TW); else gy = ld4(dy + ((int64_t)b * TW + tp) * C + col);
        pool_grad<W>(z, gy, g);
#pragma unroll
        for (int i = 0; i < W; ++i) st4(dx + (row + i) * C + col, gr * (g[i] - kb - h[i] * kg));
      } else {
        for (int i = 0; W * tp + i < T; ++i) {
          const float4 ha = bn_xhat(k, ld4(x + (row + i) * C + col));
          st4(dx + (row + i) * C + col, gr * (f4(0.f) - kb - ha * kg));
        }
      }
    } else {
      const float4 h = bn_xhat(k, ld4(x + (int64_t)u * C + col));
      const float4 g = gate(bn_act(k, h), ld4(dy + (int64_t)(u / T) * C + col) * inv_t);
      st4(dx + (int64_t)u * C + col, gr * (g - kb - h * kg));
    }
  }
}

bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t a = 0;
  for (const void* p : ps) a |= (uintptr_t)p;
  return (a & 15) == 0;
}
int slabs(int64_t units) { return (int)((units + kSlab - 1) / kSlab); }
size_t partial_bytes(int64_t units, int C) { return (size_t)slabs(units) * 2 * (size_t)C * 4; }
bool shape_ok(int B, int T, int C) { return B > 0 && T > 0 && C > 0 && (int64_t)B * T <= (int64_t)kSlab * 65535; }

// awt_op_conv1d's workspace: the planes of x [B T, Cin], then the packed planes of w [Cout, 3 Cin]
struct Conv1dWs { PlanePair x, w; size_t bytes; };
Conv1dWs conv1d_layout(void* base, int B, int T, int Cin, int Cout) {
  Carver cv(base);
  return {take_planes(cv, (size_t)B * T * Cin), take_planes(cv, (size_t)Cout * 3 * Cin), cv.bytes()};
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI (include/awt.h)
extern "C" size_t awt_op_conv1d_workspace_bytes(int B, int T, int Cin, int Cout) {
  if (B <= 0 || T <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return conv1d_layout(nullptr, B, T, Cin, Cout).bytes;
}
extern "C" int awt_op_conv1d(awt_ctx* c, const float* x, const float* w, const float* bias, float* y, int B, int T, int Cin, int Cout, int taps,
                             int terms, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(taps == 3, AWT_ERR_INVALID, "op_conv1d: taps must be 3 (kernel_size 3, padding 1, stride 1)");
  AWT_REQUIRE(terms == PREC_BF16 || terms == PREC_BF16X3 || terms == PREC_F16X3, AWT_ERR_INVALID, "op_conv1d: terms must be 1 (bf16), 3 (bf16x3) or 4 (fp16x3)");
  AWT_REQUIRE(c && x && w && y && workspace, AWT_ERR_INVALID, "op_conv1d: null argument");
  AWT_REQUIRE(B > 0 && T > 0 && (int64_t)B * T <= 0x7FFFFFFF && Cin > 0 && Cin % 64 == 0 && Cout > 0 && Cout % 128 == 0, AWT_ERR_INVALID,
              "op_conv1d: Cin % 64 == 0 and Cout % 128 == 0 required (channels a multiple of 4: pad them)");
  AWT_REQUIRE(aligned16({x, w, y, bias}) && ((uintptr_t)workspace & 255) == 0, AWT_ERR_INVALID, "op_conv1d: tensors must be 16-byte, the workspace 256-byte aligned");
  AWT_REQUIRE(ws_bytes >= awt_op_conv1d_workspace_bytes(B, T, Cin, Cout), AWT_ERR_WORKSPACE, "op_conv1d: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int M = B * T, K = 3 * Cin;
  const Conv1dWs ws = conv1d_layout(workspace, B, T, Cin, Cout);
  bf16_t *const xh = ws.x.hi, *const xl = ws.x.lo, *const wh = ws.w.hi, *const wl = ws.w.lo;
  // terms 4: the same three products on fp16 hi + lo planes -- 22 significant bits per operand where the bf16 pair has 16, for operands inside
  // fp16's range (the forward's activations and weights; gradients are not: they take the bf16 planes).  BatchNorm + ReLU + max-pool downstream
  // are discontinuous, so the forward's last bits decide masks: this is the format the model's forward convs run in (cnn_classifier.py).
  const bool two = terms != PREC_BF16;
  int rc = terms == PREC_F16X3 ? launch_split_planes(c, x, (int64_t)M * Cin, 1.0f, terms, kF8Act, xh, xl, nullptr, nullptr, s)
                               : launch_split_f32(c, x, (int64_t)M * Cin, 1.0f, PlanePair{xh, two ? xl : nullptr}, s);
  if (rc) return rc;
  rc = launch_pack_weight(c, w, Cout, Cin, 3, K, 0, 0, 1.0f, wh, two ? wl : nullptr, nullptr, terms, s); if (rc) return rc;   // k = tap Cin + ci
  GemmSeg sg[3];
  for (int tap = 0; tap < 3; ++tap) {     // output frame t of a clip reads frame t + tap - 1 of the SAME clip; outside [0, T) reads as zero (the padding)
    sg[tap] = gemm_seg_plain(xh, two ? xl : nullptr, Cin, wh, two ? wl : nullptr, K / 32, tap * Cin / 32, Cin, M);
    sg[tap].rows_out = T; sg[tap].rows_in = T; sg[tap].row_mul = 1; sg[tap].row_add = tap - 1;
  }
  GemmOut o{}; o.f32 = y; o.ldo = Cout; o.bias = bias; o.n_valid = Cout;
  return launch_gemm(c, M, Cout, sg, 3, terms, EPI_F32, o, s);
}

extern "C" size_t awt_op_batchnorm_stats_workspace_bytes(int M, int C) { return (M <= 0 || C <= 0) ? 0 : partial_bytes(M, C); }
extern "C" int awt_op_batchnorm_stats(awt_ctx* c, const float* x, int M, int C, float* mean, float* var, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(C > 0 && C % 4 == 0, AWT_ERR_INVALID, "op_batchnorm_stats: C must be a positive multiple of 4");
  AWT_REQUIRE(c && x && mean && var && workspace && shape_ok(M, 1, C), AWT_ERR_INVALID, "op_batchnorm_stats: null or empty argument");
  AWT_REQUIRE(aligned16({x, mean, var, workspace}), AWT_ERR_INVALID, "op_batchnorm_stats: tensors must be 16-byte aligned");
  AWT_REQUIRE(ws_bytes >= awt_op_batchnorm_stats_workspace_bytes(M, C), AWT_ERR_WORKSPACE, "op_batchnorm_stats: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nslab = slabs(M), gx = (C / 4 + kCols - 1) / kCols;
  hipLaunchKernelGGL(bn_stats_slab_kernel, dim3(gx, nslab), dim3(256), 0, s, x, M, C, (float*)workspace);
  hipLaunchKernelGGL(bn_stats_merge_kernel, dim3((C / 4 + 255) / 256), dim3(256), 0, s, (const float*)workspace, nslab, M, C, mean, var);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

namespace {
// pool codes (awt.h AWT_POOL_*): the window of the max-pool, 0 for none
int pool_window(int pool) { return pool == AWT_POOL_MAX2 ? 2 : (pool == AWT_POOL_MAX4 || pool == AWT_POOL_MAX4_MEAN) ? 4 : 0; }
bool pool_ok(int pool, int T) { return pool == AWT_POOL_MEAN || (pool_window(pool) > 0 && T >= pool_window(pool)); }
}  // namespace

extern "C" int awt_op_bn_relu_pool(awt_ctx* c, const float* x, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                                   float* y, int B, int T, int C, int pool, void* stream) {
  AWT_REQUIRE(C > 0 && C % 4 == 0, AWT_ERR_INVALID, "op_bn_relu_pool: C must be a positive multiple of 4");
  AWT_REQUIRE(pool_ok(pool, T), AWT_ERR_INVALID,
              "op_bn_relu_pool: pool must be 0 (mean over T), 2 (max over frame pairs, T >= 2), 4 (max over 4 frames, T >= 4) or 5 (4, then the mean)");
  AWT_REQUIRE(c && x && mean && var && gamma && beta && y && shape_ok(B, T, C) && eps >= 0.f, AWT_ERR_INVALID, "op_bn_relu_pool: null or empty argument");
  AWT_REQUIRE(aligned16({x, mean, var, gamma, beta, y}), AWT_ERR_INVALID, "op_bn_relu_pool: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int gx = (C / 4 + kCols - 1) / kCols;
  if (pool == AWT_POOL_MAX2 || pool == AWT_POOL_MAX4) {
    const int TW = T / pool_window(pool), U = B * TW;
    if (pool == AWT_POOL_MAX2) hipLaunchKernelGGL(bn_relu_maxpool_kernel<2>, dim3(gx, slabs(U)), dim3(256), 0, s, x, mean, var, gamma, beta, eps, y, U, T, TW, C);
    else hipLaunchKernelGGL(bn_relu_maxpool_kernel<4>, dim3(gx, slabs(U)), dim3(256), 0, s, x, mean, var, gamma, beta, eps, y, U, T, TW, C);
  } else {
    AWT_REQUIRE((B + kLanes - 1) / kLanes <= 65535, AWT_ERR_INVALID, "op_bn_relu_pool: too many clips");
    const dim3 grid(gx, (B + kLanes - 1) / kLanes);
    if (pool == AWT_POOL_MEAN) hipLaunchKernelGGL(bn_relu_avgpool_kernel, grid, dim3(256), 0, s, x, mean, var, gamma, beta, eps, y, B, T, C);
    else hipLaunchKernelGGL(bn_relu_maxpool_mean_kernel<4>, grid, dim3(256), 0, s, x, mean, var, gamma, beta, eps, y, B, T, T / 4, C);
  }
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" size_t awt_op_bn_relu_pool_backward_workspace_bytes(int B, int T, int C) {
  return (B <= 0 || T <= 0 || C <= 0) ? 0 : partial_bytes((int64_t)B * T, C);       // covers every pooling (the max-pools have fewer units)
}
namespace {
template <int W, bool MEAN>
void launch_pool_backward(hipStream_t s, const float* dy, const float* x, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                          float* dx, float* dgamma, float* dbeta, int B, int T, int C, float* partial) {
  const int gx = (C / 4 + kCols - 1) / kCols, gsum = (C / 4 + 255) / 256;
  const int TW = W > 0 ? T / (W > 0 ? W : 1) : T / 2;
  const int Ur = W > 0 ? B * TW : B * T, Ua = W > 0 ? B * ((T + W - 1) / (W > 0 ? W : 1)) : B * T;
  const float inv_m = 1.0f / ((float)B * (float)T);
  hipLaunchKernelGGL((bn_pool_bwd_reduce_kernel<W, MEAN>), dim3(gx, slabs(Ur)), dim3(256), 0, s, dy, x, mean, var, gamma, beta, eps, Ur, T, TW, C, partial);
  hipLaunchKernelGGL(bn_pool_bwd_sum_kernel, dim3(gsum), dim3(256), 0, s, (const float*)partial, slabs(Ur), C, dgamma, dbeta);
  hipLaunchKernelGGL((bn_pool_bwd_apply_kernel<W, MEAN>), dim3(gx, slabs(Ua)), dim3(256), 0, s, dy, x, mean, var, gamma, beta, eps, (const float*)dgamma,
                     (const float*)dbeta, Ua, T, TW, C, inv_m, dx);
}
}  // namespace
extern "C" int awt_op_bn_relu_pool_backward(awt_ctx* c, const float* dy, const float* x, const float* mean, const float* var, const float* gamma,
                                            const float* beta, float eps, float* dx, float* dgamma, float* dbeta, int B, int T, int C, int pool,
                                            void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(C > 0 && C % 4 == 0, AWT_ERR_INVALID, "op_bn_relu_pool_backward: C must be a positive multiple of 4");
  AWT_REQUIRE(pool_ok(pool, T), AWT_ERR_INVALID, "op_bn_relu_pool_backward: pool must be 0, 2 (T >= 2), 4 or 5 (T >= 4)");
  AWT_REQUIRE(c && dy && x && mean && var && gamma && beta && dx && dgamma && dbeta && workspace && shape_ok(B, T, C) && eps >= 0.f, AWT_ERR_INVALID,
              "op_bn_relu_pool_backward: null or empty argument");
  AWT_REQUIRE(aligned16({dy, x, mean, var, gamma, beta, dx, dgamma, dbeta, workspace}), AWT_ERR_INVALID, "op_bn_relu_pool_backward: tensors must be 16-byte aligned");
  AWT_REQUIRE(ws_bytes >= awt_op_bn_relu_pool_backward_workspace_bytes(B, T, C), AWT_ERR_WORKSPACE, "op_bn_relu_pool_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  if (pool == AWT_POOL_MAX2) launch_pool_backward<2, false>(s, dy, x, mean, var, gamma, beta, eps, dx, dgamma, dbeta, B, T, C, partial);
  else if (pool == AWT_POOL_MAX4) launch_pool_backward<4, false>(s, dy, x, mean, var, gamma, beta, eps, dx, dgamma, dbeta, B, T, C, partial);
  else if (pool == AWT_POOL_MAX4_MEAN) launch_pool_backward<4, true>(s, dy, x, mean, var, gamma, beta, eps, dx, dgamma, dbeta, B, T, C, partial);
  else launch_pool_backward<0, false>(s, dy, x, mean, var, gamma, beta, eps, dx, dgamma, dbeta, B, T, C, partial);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

// ------------------------------------------------------------------------------------------------ framed Conv1d(1, Cout, kernel, stride) on the raw waveform
// DESIGN section 4.10.  y[b, t, co] = bias[co] + sum_k x[b, t stride + k] w[co, k] as a GEMM of frames x taps on the exact-fp32 MFMA
// (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain that starts at the bias).  A workgroup of 4 waves owns kFramedRows consecutive frames of one
// clip and stages, once, the samples they cover and the whole weight in LDS:
//   samples  as rows of `stride` floats at a pitch of stride + 4: frame f, tap k = j stride + r  is  sx[(f + j) (stride + 4) + r].  The MFMA's B operand
//            is lane (frame l & 15, k = 4 step + (l >> 4)); with pitch / 4 odd (stride % 8 == 0) the 16 frames start on the 16 different multiples
//            of 4 banks and the 4 k fill them: 64 lanes, 64 banks.  At the natural pitch (stride = 16) frames 0, 4, 8, 12 would share a bank.
//   weights  [Cout][kernel + 4]: the A operand is lane (channel l & 15, k = 4 step + (l >> 4)), conflict-free for the same reason.
// A = weights, B = frames puts 4 consecutive channels of ONE frame in a lane's accumulator (D row = channel 4 (l >> 4) + reg, column = frame): a
// float4 store per lane, 64 contiguous bytes per frame and channel tile.  A wave owns 2 frame tiles x CT channel tiles = 2 CT independent accumulators.
namespace {
constexpr int kFramedRows = 128;          // output frames per workgroup (waveform_classifier.FRAMED_ROWS_PER_WORKGROUP)
constexpr int kFramedLds = 64 * 1024;     // the staging may take this much LDS

size_t framed_lds_bytes(int kernel, int stride, int Cout) {
  return ((size_t)(kFramedRows + kernel / stride - 1) * (stride + 4) + (size_t)Cout * (kernel + 4)) * 4;
}

template <int CT>
__global__ __launch_bounds__(256) void conv1d_framed_kernel(const float* __restrict__ x, int64_t x_pitch, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ y, int T1, int kernel, int stride, int Cout) {
  extern __shared__ float4 framed_lds[];
  const int taps = kernel / stride, P = stride + 4, WP = kernel + 4;
  float* sx = reinterpret_cast<float*>(framed_lds);
  float* sw = sx + (kFramedRows + taps - 1) * P;
  const int b = blockIdx.y, f0 = blockIdx.x * kFramedRows, rows = min(kFramedRows, T1 - f0);
  const float* xs = x + (int64_t)b * x_pitch + (int64_t)f0 * stride;
  const int n_valid = stride * (rows - 1) + kernel;            // the samples this tile's frames cover: all inside the clip; a multiple of 4
  for (int p = 4 * threadIdx.x; p < (kFramedRows + taps - 1) * stride; p += 4 * 256) {
    const int r = p / stride, col = p - r * stride;
    st4(sx + r * P + col, p < n_valid ? ld4(xs + p) : f4(0.f));
  }
  for (int p = 4 * threadIdx.x; p < Cout * kernel; p += 4 * 256) {
    const int co = p / kernel, k = p - co * kernel;
    st4(sw + co * WP + k, ld4(w + p));
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
  const int fw = wave * 32;                                    // this wave's frames: fw + 16 ft + j
  if (fw >= rows) return;
  const float* bx = sx + (fw + j) * P + g;
  for (int co0 = 0; co0 < Cout; co0 += 16 * CT) {
    f32x4 acc[2][CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const float4 bv = ld4(bias + co0 + 16 * ct + 4 * g);
      acc[0][ct] = acc[1][ct] = f32x4{bv.x, bv.y, bv.z, bv.w};
    }
    const float* aw = sw + (co0 + j) * WP + g;
    auto k_step = [&](int k, int xo) {                            // taps k ... k + 3: 2 + CT LDS reads, 2 CT MFMAs
      const float b0 = bx[xo], b1 = bx[16 * P + xo];
      float a[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) a[ct] = aw[16 * ct * WP + k];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct], b0, acc[0][ct], 0, 0, 0);
        acc[1][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ct], b1, acc[1][ct], 0, 0, 0);
      }
    };
    for (int tap = 0; tap < taps; ++tap)
      for (int c0 = 0; c0 < stride; c0 += 8) {                    // stride % 8 == 0: two k-steps per trip, in k order
        k_step(tap * stride + c0, tap * P + c0);
        k_step(tap * stride + c0 + 4, tap * P + c0 + 4);
      }
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
      const int f = fw + 16 * ft + j;
      if (f >= rows) continue;
      float* yo = y + ((int64_t)b * T1 + f0 + f) * Cout + co0 + 4 * g;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) st4(yo + 16 * ct, make_float4(acc[ft][ct][0], acc[ft][ct][1], acc[ft][ct][2], acc[ft][ct][3]));
    }
  }
}
// the LDS attribute is set once per device to the LARGEST size a call may ask for: the size of a call depends on (kernel, stride, Cout)
template <auto Kernel, class... Args>
int launch_framed(dim3 grid, int lds, hipStream_t s, const Args&... args) {
  AWT_ONCE_PER_DEVICE(AWT_HIP_CHECK(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kFramedLds)));
  hipLaunchKernelGGL(Kernel, grid, dim3(256), lds, s, args...);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}
}  // namespace

extern "C" int awt_op_conv1d_framed(awt_ctx* c, const float* x, int64_t x_pitch, const float* w, const float* bias, float* y, int B, int n_samples,
                                    int kernel, int stride, int Cout, void* stream) {
  AWT_REQUIRE(stride > 0 && stride % 8 == 0, AWT_ERR_INVALID, "op_conv1d_framed: stride must be a positive multiple of 8");
  AWT_REQUIRE(kernel > 0 && kernel % stride == 0, AWT_ERR_INVALID, "op_conv1d_framed: kernel must be a positive multiple of the stride");
  AWT_REQUIRE(n_samples >= kernel, AWT_ERR_INVALID, "op_conv1d_framed: n_samples must be at least kernel (no padding)");
  AWT_REQUIRE(Cout > 0 && Cout % 16 == 0 && framed_lds_bytes(kernel, stride, Cout) <= (size_t)kFramedLds, AWT_ERR_INVALID,
              "op_conv1d_framed: Cout must be a positive multiple of 16, and weights and staged samples must fit 64 KiB of LDS");
  AWT_REQUIRE(c && x && w && bias && y, AWT_ERR_INVALID, "op_conv1d_framed: null argument");
  AWT_REQUIRE(B > 0 && B <= 65535 && x_pitch >= n_samples && x_pitch % 4 == 0, AWT_ERR_INVALID,
              "op_conv1d_framed: 1 <= B <= 65535 and a clip pitch >= n_samples that is a multiple of 4 required");
  AWT_REQUIRE(aligned16({x, w, bias, y}), AWT_ERR_INVALID, "op_conv1d_framed: tensors must be 16-byte aligned");
  const int T1 = (n_samples - kernel) / stride + 1;
  const dim3 grid((T1 + kFramedRows - 1) / kFramedRows, B);
  const int lds = (int)framed_lds_bytes(kernel, stride, Cout);
  hipStream_t s = (hipStream_t)stream;
  if (Cout % 64 == 0) return launch_framed<conv1d_framed_kernel<4>>(grid, lds, s, x, x_pitch, w, bias, y, T1, kernel, stride, Cout);
  if (Cout % 32 == 0) return launch_framed<conv1d_framed_kernel<2>>(grid, lds, s, x, x_pitch, w, bias, y, T1, kernel, stride, Cout);
  return launch_framed<conv1d_framed_kernel<1>>(grid, lds, s, x, x_pitch, w, bias, y, T1, kernel, stride, Cout);
}
