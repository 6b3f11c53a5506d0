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

constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }

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
__device__ __forceinline__ float4 relu4(const float4 z) { return max4(z, f4(0.f)); }
__device__ __forceinline__ float4 gate(const float4 z, const float4 g) {           // g where z > 0: ReLU's derivative
  return make_float4(z.x > 0.f ? g.x : 0.f, z.y > 0.f ? g.y : 0.f, z.z > 0.f ? g.z : 0.f, z.w > 0.f ? g.w : 0.f);
}
// Gradient of max(relu(za), relu(zb)) with respect to za and zb.  The winner is the larger pre-ReLU value, the first on a tie.  After the ReLU a
// tie between two DIFFERENT inputs can only be 0 = 0, where ReLU's derivative is zero whichever index is named, so the kernel would not have to
// reproduce torch's first-index tie-break; `>=` costs nothing and also covers equal positive values (a constant channel ties at beta).
__device__ __forceinline__ void pool2_grad(const float4 za, const float4 zb, const float4 g, float4& ga, float4& gb) {
  ga = make_float4(za.x >= zb.x ? g.x : 0.f, za.y >= zb.y ? g.y : 0.f, za.z >= zb.z ? g.z : 0.f, za.w >= zb.w ? g.w : 0.f);
  gb = gate(zb, g - ga);
  ga = gate(za, ga);
}

// pool = 2: unit u = (clip b, pooled frame t2) reads rows b T + 2 t2 and + 1, writes row u of y [B (T / 2), C]; an odd T's last frame is not read.
__global__ __launch_bounds__(256) void bn_relu_maxpool_kernel(const float* __restrict__ x, const float* mean, const float* var, const float* gamma,
                                                              const float* beta, float eps, float* __restrict__ y, int U, int T, int T2, int C) {
  const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
  const int col = (blockIdx.x * kCols + tx) * 4;
  if (col >= C) return;
  const BnCoef k = bn_coef(mean, var, gamma, beta, eps, col);
  const int u0 = blockIdx.y * kSlab + ty;
#pragma unroll 4
  for (int j = 0; j < kPerLane; ++j) {
    const int u = u0 + kLanes * j;
    if (u >= U) break;
    const int b = u / T2, t2 = u - b * T2;
    const float* p = x + ((int64_t)b * T + 2 * t2) * C + col;
    const float4 za = bn_act(k, bn_xhat(k, ld4(p))), zb = bn_act(k, bn_xhat(k, ld4(p + C)));
    st4(y + (int64_t)u * C + col, relu4(max4(za, zb)));
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

// Backward, launch 1: partial[slab][0][C] = sum dz, partial[slab][1][C] = sum dz xhat over the slab's units, dz the gradient at the BatchNorm
// output.  POOL2: unit = a pooled frame (two rows of x, one of dy; the frame an odd T drops has dz = 0 and adds nothing); else unit = a row of x
// with dz = relu'(z) dy[clip] / T.
template <bool POOL2>
__global__ __launch_bounds__(256) void bn_pool_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* mean, const float* var,
                                                                 const float* gamma, const float* beta, float eps, int U, int T, int T2, int C,
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
      if constexpr (POOL2) {
        const int b = u / T2, t2 = u - b * T2;
        const float* p = x + ((int64_t)b * T + 2 * t2) * C + col;
        const float4 ha = bn_xhat(k, ld4(p)), hb = bn_xhat(k, ld4(p + C));
        float4 ga, gb;
        pool2_grad(bn_act(k, ha), bn_act(k, hb), ld4(dy + (int64_t)u * C + col), ga, gb);
        a1 = a1 + ga + gb;
        a2 = a2 + ga * ha + gb * hb;
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
// Backward, launch 3: dx = gamma rstd (dz - dbeta / M - xhat dgamma / M) for EVERY row of x, M = B T.  POOL2: unit = (clip, frame pair p < ceil(T / 2));
// the lone last frame of an odd T has dz = 0 but still receives the two mean terms.
template <bool POOL2>
__global__ __launch_bounds__(256) void bn_pool_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* mean, const float* var,
                                                                const float* gamma, const float* beta, float eps, const float* dgamma, const float* dbeta,
                                                                int U, int T, int T2, int C, float inv_m, float* __restrict__ dx) {
  const int tx = threadIdx.x & (kCols - 1), ty = threadIdx.x / kCols;
  const int col = (blockIdx.x * kCols + tx) * 4;
  if (col >= C) return;
  const BnCoef k = bn_coef(mean, var, gamma, beta, eps, col);
  const float4 kb = ld4(dbeta + col) * inv_m, kg = ld4(dgamma + col) * inv_m, gr = k.gamma * k.rstd;
  const float inv_t = 1.0f / (float)T;
  const int Tp = (T + 1) / 2;
  const int u0 = blockIdx.y * kSlab + ty;
#pragma unroll 2
  for (int j = 0; j < kPerLane; ++j) {
    const int u = u0 + kLanes * j;
    if (u >= U) break;
    if constexpr (POOL2) {
      const int b = u / Tp, tp = u - b * Tp;
      const int64_t row = (int64_t)b * T + 2 * tp;
      const float4 ha = bn_xhat(k, ld4(x + row * C + col));
      if (tp < T2) {
        const float4 hb = bn_xhat(k, ld4(x + (row + 1) * C + col));
        float4 ga, gb;
        pool2_grad(bn_act(k, ha), bn_act(k, hb), ld4(dy + ((int64_t)b * T2 + tp) * C + col), ga, gb);
        st4(dx + row * C + col, gr * (ga - kb - ha * kg));
        st4(dx + (row + 1) * C + col, gr * (gb - kb - hb * kg));
      } else {
        st4(dx + row * C + col, gr * (f4(0.f) - kb - ha * kg));
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

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI (include/awt.h)
extern "C" size_t awt_op_conv1d_workspace_bytes(int B, int T, int Cin, int Cout) {
  if (B <= 0 || T <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return 2 * align_up((size_t)B * T * Cin * 2) + 2 * align_up((size_t)Cout * 3 * Cin * 2);       // x planes, packed w planes
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
  char* base = (char*)workspace;
  const size_t xb = align_up((size_t)M * Cin * 2), wb = align_up((size_t)Cout * K * 2);
  bf16_t* xh = (bf16_t*)base; bf16_t* xl = (bf16_t*)(base + xb);
  bf16_t* wh = (bf16_t*)(base + 2 * xb); bf16_t* wl = (bf16_t*)(base + 2 * xb + wb);
  // terms 4: the same three products on fp16 hi + lo planes -- 22 significant bits per operand where the bf16 pair has 16, for operands inside
  // fp16's range (the forward's activations and weights; gradients are not: they take the bf16 planes).  BatchNorm + ReLU + max-pool downstream
  // are discontinuous, so the forward's last bits decide masks: this is the format the model's forward convs run in (cnn_classifier.py).
  const bool two = terms != PREC_BF16;
  int rc = terms == PREC_F16X3 ? launch_split_planes(c, x, (int64_t)M * Cin, 1.0f, terms, kF8Act, xh, xl, nullptr, nullptr, s)
                               : launch_split_f32(c, x, (int64_t)M * Cin, 1.0f, xh, two ? xl : nullptr, s);
  if (rc) return rc;
  rc = launch_pack_weight(c, w, Cout, Cin, 3, K, 0, 0, 1.0f, wh, two ? wl : nullptr, nullptr, terms, s); if (rc) return rc;   // k = tap Cin + ci
  GemmSeg sg[3];
  for (int tap = 0; tap < 3; ++tap) {     // output frame t of a clip reads frame t + tap - 1 of the SAME clip; outside [0, T) reads as zero (the padding)
    GemmSeg g{};
    g.a_hi = xh; g.a_lo = two ? xl : nullptr; g.lda = Cin;
    g.w_hi = wh; g.w_lo = two ? wl : nullptr; g.w_ksteps = K / 32; g.w_k0 = tap * Cin / 32; g.K = Cin;
    g.rows_out = T; g.rows_in = T; g.row_mul = 1; g.row_add = tap - 1;
    sg[tap] = g;
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

extern "C" int awt_op_bn_relu_pool(awt_ctx* c, const float* x, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                                   float* y, int B, int T, int C, int pool, void* stream) {
  AWT_REQUIRE(C > 0 && C % 4 == 0, AWT_ERR_INVALID, "op_bn_relu_pool: C must be a positive multiple of 4");
  AWT_REQUIRE(pool == 0 || (pool == 2 && T >= 2), AWT_ERR_INVALID, "op_bn_relu_pool: pool must be 2 (max over frame pairs, T >= 2) or 0 (mean over T)");
  AWT_REQUIRE(c && x && mean && var && gamma && beta && y && shape_ok(B, T, C) && eps >= 0.f, AWT_ERR_INVALID, "op_bn_relu_pool: null or empty argument");
  AWT_REQUIRE(aligned16({x, mean, var, gamma, beta, y}), AWT_ERR_INVALID, "op_bn_relu_pool: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int gx = (C / 4 + kCols - 1) / kCols;
  if (pool == 2) {
    const int T2 = T / 2, U = B * T2;
    hipLaunchKernelGGL(bn_relu_maxpool_kernel, dim3(gx, slabs(U)), dim3(256), 0, s, x, mean, var, gamma, beta, eps, y, U, T, T2, C);
  } else {
    AWT_REQUIRE((B + kLanes - 1) / kLanes <= 65535, AWT_ERR_INVALID, "op_bn_relu_pool: too many clips");
    hipLaunchKernelGGL(bn_relu_avgpool_kernel, dim3(gx, (B + kLanes - 1) / kLanes), dim3(256), 0, s, x, mean, var, gamma, beta, eps, y, B, T, C);
  }
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" size_t awt_op_bn_relu_pool_backward_workspace_bytes(int B, int T, int C) {
  return (B <= 0 || T <= 0 || C <= 0) ? 0 : partial_bytes((int64_t)B * T, C);       // covers both poolings (pool = 2 has half the units)
}
extern "C" int awt_op_bn_relu_pool_backward(awt_ctx* c, const float* dy, const float* x, const float* mean, const float* var, const float* gamma,
                                            const float* beta, float eps, float* dx, float* dgamma, float* dbeta, int B, int T, int C, int pool,
                                            void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(C > 0 && C % 4 == 0, AWT_ERR_INVALID, "op_bn_relu_pool_backward: C must be a positive multiple of 4");
  AWT_REQUIRE(pool == 0 || (pool == 2 && T >= 2), AWT_ERR_INVALID, "op_bn_relu_pool_backward: pool must be 2 (T >= 2) or 0");
  AWT_REQUIRE(c && dy && x && mean && var && gamma && beta && dx && dgamma && dbeta && workspace && shape_ok(B, T, C) && eps >= 0.f, AWT_ERR_INVALID,
              "op_bn_relu_pool_backward: null or empty argument");
  AWT_REQUIRE(aligned16({dy, x, mean, var, gamma, beta, dx, dgamma, dbeta, workspace}), AWT_ERR_INVALID, "op_bn_relu_pool_backward: tensors must be 16-byte aligned");
  AWT_REQUIRE(ws_bytes >= awt_op_bn_relu_pool_backward_workspace_bytes(B, T, C), AWT_ERR_WORKSPACE, "op_bn_relu_pool_backward: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int gx = (C / 4 + kCols - 1) / kCols, gsum = (C / 4 + 255) / 256, T2 = T / 2;
  const float inv_m = 1.0f / ((float)B * (float)T);
  float* partial = (float*)workspace;
  if (pool == 2) {
    const int Ur = B * T2, Ua = B * ((T + 1) / 2);
    hipLaunchKernelGGL(bn_pool_bwd_reduce_kernel<true>, dim3(gx, slabs(Ur)), dim3(256), 0, s, dy, x, mean, var, gamma, beta, eps, Ur, T, T2, C, partial);
    hipLaunchKernelGGL(bn_pool_bwd_sum_kernel, dim3(gsum), dim3(256), 0, s, (const float*)partial, slabs(Ur), C, dgamma, dbeta);
    hipLaunchKernelGGL(bn_pool_bwd_apply_kernel<true>, dim3(gx, slabs(Ua)), dim3(256), 0, s, dy, x, mean, var, gamma, beta, eps, (const float*)dgamma,
                       (const float*)dbeta, Ua, T, T2, C, inv_m, dx);
  } else {
    const int U = B * T;
    hipLaunchKernelGGL(bn_pool_bwd_reduce_kernel<false>, dim3(gx, slabs(U)), dim3(256), 0, s, dy, x, mean, var, gamma, beta, eps, U, T, T2, C, partial);
    hipLaunchKernelGGL(bn_pool_bwd_sum_kernel, dim3(gsum), dim3(256), 0, s, (const float*)partial, slabs(U), C, dgamma, dbeta);
    hipLaunchKernelGGL(bn_pool_bwd_apply_kernel<false>, dim3(gx, slabs(U)), dim3(256), 0, s, dy, x, mean, var, gamma, beta, eps, (const float*)dgamma,
                       (const float*)dbeta, U, T, T2, C, inv_m, dx);
  }
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}
