// The row operators of a Qwen3 decoder layer that the library did not have -- gfx950.  All fp32 in, fp32 out, on the caller's stream, HBM-bound.
//   awt_op_rmsnorm        y = gamma x rsqrt(mean(x^2) + eps)                      one wave per row, x read twice (the second time from cache)
//   awt_op_qk_norm_rope   per-head RMSNorm of q and k, rotary embedding, q to its own buffer, k and v into the decode cache: one wave per (row, head)
//   awt_op_silu_mul       y = silu(gate) * up over one [M, 2 I] gate | up GEMM output   16-byte accesses
// The causal attention of the layer is the CAUSAL variant of csrc/cross_attention.hip's forward.  (music2midi.Qwen3Decoder)
// And their backward, for training through the decoder, further down:
//   awt_op_rmsnorm_backward / _param_grad   dx = [dres +] r u - x r^3 mean(x u), u = gamma dy;  dgamma = sum_m dy x r in slabs, a fixed order
//   awt_op_silu_mul_backward                dgate | dup from the forward's gate | up and dy
//   awt_op_qk_norm_rope_backward            transposed rotation, per-head norm backward, dv copied: one wave per (row, head); the gains' gradients in slabs
#include <algorithm>
#include "common.h"

namespace {

constexpr int QD = 128;            // head_dim
constexpr int QTHREADS = 256;      // four waves: four rows (rmsnorm) / four (row, head) pairs (qk_norm_rope) per workgroup

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------ RMSNorm
// Lane l sums the squares of the float4 pieces l, l + 64, ... of its row in order, then one butterfly over the wave: a fixed order, so two runs agree.
__global__ __launch_bounds__(QTHREADS) void rmsnorm_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ gamma, float* __restrict__ y, int64_t ldy,
                                                           int M, int d, float eps) {
  const int row = blockIdx.x * (QTHREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;                                            // wave-uniform
  const float* xr = x + (int64_t)row * ldx;
  float* yr = y + (int64_t)row * ldy;
  float ss = 0.f;
  for (int c = 4 * lane; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c);
    ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
  }
  const float r = __builtin_amdgcn_rsqf(wave_sum(ss) / (float)d + eps);
  for (int c = 4 * lane; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c), g = *reinterpret_cast<const float4*>(gamma + c);
    *reinterpret_cast<float4*>(yr + c) = make_float4(g.x * (v.x * r), g.y * (v.y * r), g.z * (v.z * r), g.w * (v.w * r));
  }
}

// ------------------------------------------------------------------------------------------------ q / k norm + rotary embedding + cache append
struct RopeArgs {
  const float* qkv; int64_t ld;                  // [B Lq, (Hq + 2 Hkv) 128]: q heads | k heads | v heads
  const float *q_gamma, *k_gamma;                // [128] each
  const float *cos, *sin;                        // [Tmax, 64]
  const int32_t* positions;                      // [B Lq]
  float* q_out; int64_t ldq;
  float *k_cache, *v_cache; int64_t ldkv, kvbs;
  int rows, Lq, Hq, Hkv, Tmax;
  float eps;
};
// Lane l holds dims l and l + 64 of its head: HF's rotate_half pairs exactly those two, so the rotation needs no other lane, and the head's sum of squares is
// one wave reduction.  A position outside [0, Tmax) is clamped (the call cannot fail without a synchronisation, and it never writes outside the cache).
__global__ __launch_bounds__(QTHREADS) void qk_norm_rope_kernel(RopeArgs a) {
  const int heads = a.Hq + 2 * a.Hkv;
  const int64_t w = (int64_t)blockIdx.x * (QTHREADS / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= (int64_t)a.rows * heads) return;                        // wave-uniform
  const int row = (int)(w / heads), head = (int)(w - (int64_t)row * heads), b = row / a.Lq;
  const int pos = min(max(a.positions[row], 0), a.Tmax - 1);
  const float* src = a.qkv + (int64_t)row * a.ld + QD * head;
  const float x0 = src[lane], x1 = src[lane + 64];
  if (head >= a.Hq + a.Hkv) {                                      // v: copied
    float* dst = a.v_cache + (int64_t)b * a.kvbs + (int64_t)pos * a.ldkv + QD * (head - a.Hq - a.Hkv);
    dst[lane] = x0; dst[lane + 64] = x1;
    return;
  }
  const bool is_q = head < a.Hq;
  const float* g = is_q ? a.q_gamma : a.k_gamma;
  const float r = __builtin_amdgcn_rsqf(wave_sum(fmaf(x0, x0, x1 * x1)) * (1.0f / QD) + a.eps);
  const float n0 = g[lane] * (x0 * r), n1 = g[lane + 64] * (x1 * r);
  const float cs = a.cos[(int64_t)pos * 64 + lane], sn = a.sin[(int64_t)pos * 64 + lane];
  float* dst = is_q ? a.q_out + (int64_t)row * a.ldq + QD * head : a.k_cache + (int64_t)b * a.kvbs + (int64_t)pos * a.ldkv + QD * (head - a.Hq);
  dst[lane] = fmaf(n0, cs, -(n1 * sn));                            // x cos + rotate_half(x) sin, rotate_half(x) = (-x[64:], x[:64])
  dst[lane + 64] = fmaf(n1, cs, n0 * sn);
}

// ------------------------------------------------------------------------------------------------ SwiGLU's element-wise half
__global__ __launch_bounds__(QTHREADS) void silu_mul_kernel(const float* __restrict__ gu, int64_t ld, float* __restrict__ y, int64_t ldy, int M, int I) {
  const int i4 = I >> 2;
  const int64_t n = (int64_t)M * i4;
  for (int64_t idx = (int64_t)blockIdx.x * QTHREADS + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * QTHREADS) {
    const int64_t m = idx / i4; const int c = 4 * (int)(idx - m * i4);
    const float4 g = *reinterpret_cast<const float4*>(gu + m * ld + c), u = *reinterpret_cast<const float4*>(gu + m * ld + I + c);
    const float gv[4] = {g.x, g.y, g.z, g.w}, uv[4] = {u.x, u.y, u.z, u.w};
    float o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = gv[t] / (1.0f + __expf(-gv[t])) * uv[t];
    *reinterpret_cast<float4*>(y + m * ldy + c) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

// ================================================================================================ backward operators (training through the decoder)
// ------------------------------------------------------------------------------------------------ RMSNorm backward
// With r = rsqrt(mean(x^2) + eps) and u = gamma dy:  dx = [dres +] r u - x r^3 mean(x u).  One wave per row as in the forward; the two row sums (x^2, x u) share
// the first pass, each a per-lane chain in column order and one butterfly.
__global__ __launch_bounds__(QTHREADS) void rmsnorm_bwd_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ x, int64_t ldx,
                                                               const float* __restrict__ gamma, const float* dres, float* dx, int64_t lddx, int M, int d, float eps) {
  const int row = blockIdx.x * (QTHREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;                                            // wave-uniform
  const float* xr = x + (int64_t)row * ldx;
  const float* gr = dy + (int64_t)row * lddy;
  float ss = 0.f, xu = 0.f;
  for (int c = 4 * lane; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c), g = *reinterpret_cast<const float4*>(gamma + c), y = *reinterpret_cast<const float4*>(gr + c);
    ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
    xu = fmaf(v.x, g.x * y.x, xu); xu = fmaf(v.y, g.y * y.y, xu); xu = fmaf(v.z, g.z * y.z, xu); xu = fmaf(v.w, g.w * y.w, xu);
  }
  const float r = __builtin_amdgcn_rsqf(wave_sum(ss) / (float)d + eps);
  const float coef = r * r * r * (wave_sum(xu) / (float)d);
  const float* rr = dres ? dres + (int64_t)row * lddx : nullptr;
  float* outr = dx + (int64_t)row * lddx;
  for (int c = 4 * lane; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c), g = *reinterpret_cast<const float4*>(gamma + c), y = *reinterpret_cast<const float4*>(gr + c);
    float4 o = make_float4(fmaf(-v.x, coef, r * (g.x * y.x)), fmaf(-v.y, coef, r * (g.y * y.y)), fmaf(-v.z, coef, r * (g.z * y.z)), fmaf(-v.w, coef, r * (g.w * y.w)));
    if (rr) { const float4 e = *reinterpret_cast<const float4*>(rr + c); o.x += e.x; o.y += e.y; o.z += e.z; o.w += e.w; }
    *reinterpret_cast<float4*>(outr + c) = o;
  }
}

// ------------------------------------------------------------------------------------------------ RMSNorm gain gradient: dgamma[j] = sum_m dy[m, j] x[m, j] r_m
// Three launches: r_m per row (one wave per row, the forward's sum), slabs of kGainSlab rows summed top to bottom by a thread per column, the slabs added in slab
// order -- the scheme of awt_op_column_sums_ld, so two runs give the same bits.
constexpr int kGainSlab = 256;
__global__ __launch_bounds__(QTHREADS) void rms_rstd_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ rstd, int M, int d, float eps) {
  const int row = blockIdx.x * (QTHREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;                                            // wave-uniform
  const float* xr = x + (int64_t)row * ldx;
  float ss = 0.f;
  for (int c = 4 * lane; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c);
    ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
  }
  const float r = __builtin_amdgcn_rsqf(wave_sum(ss) / (float)d + eps);
  if (lane == 0) rstd[row] = r;
}
__global__ __launch_bounds__(QTHREADS) void rms_gain_slab_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ x, int64_t ldx,
                                                                 const float* __restrict__ rstd, float* __restrict__ partial, int M, int d) {
  const int c = blockIdx.x * QTHREADS + threadIdx.x;
  if (c >= d) return;
  const int r0 = blockIdx.y * kGainSlab, r1 = min(M, r0 + kGainSlab);
  float s = 0.f;
  for (int m = r0; m < r1; ++m) s = fmaf(dy[(int64_t)m * lddy + c], x[(int64_t)m * ldx + c] * rstd[m], s);
  partial[(int64_t)blockIdx.y * d + c] = s;
}
__global__ __launch_bounds__(QTHREADS) void slab_reduce_kernel(const float* __restrict__ partial, int nslab, int d, float* __restrict__ out) {
  const int c = blockIdx.x * QTHREADS + threadIdx.x;
  if (c >= d) return;
  float s = 0.f;
  for (int i = 0; i < nslab; ++i) s += partial[(int64_t)i * d + c];
  out[c] = s;
}
struct GainWs { float *rstd, *partial; size_t bytes; };
GainWs gain_layout(void* base, int M, int d) {
  Carver cv(base);
  return {cv.take<float>((size_t)M * 4), cv.take<float>((size_t)((M + kGainSlab - 1) / kGainSlab) * d * 4), cv.bytes()};
}

// ------------------------------------------------------------------------------------------------ SwiGLU backward
// With s = sigmoid(g):  dgate = dy up s (1 + g (1 - s)),  dup = dy g s.  e = exp(-|g|) never overflows; s and 1 - s are e / (1 + e) and 1 / (1 + e) in the order the
// sign of g names, so neither is a difference of nearly equal numbers.
__global__ __launch_bounds__(QTHREADS) void silu_mul_bwd_kernel(const float* __restrict__ gu, int64_t ld, const float* __restrict__ dy, int64_t lddy,
                                                                float* __restrict__ dgu, int64_t lddgu, int M, int I) {
  const int i4 = I >> 2;
  const int64_t n = (int64_t)M * i4;
  for (int64_t idx = (int64_t)blockIdx.x * QTHREADS + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * QTHREADS) {
    const int64_t m = idx / i4; const int c = 4 * (int)(idx - m * i4);
    const float4 g = *reinterpret_cast<const float4*>(gu + m * ld + c), u = *reinterpret_cast<const float4*>(gu + m * ld + I + c);
    const float4 y = *reinterpret_cast<const float4*>(dy + m * lddy + c);
    const float gv[4] = {g.x, g.y, g.z, g.w}, uv[4] = {u.x, u.y, u.z, u.w}, yv[4] = {y.x, y.y, y.z, y.w};
    float dg[4], du[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float e = __expf(-fabsf(gv[t])), inv = 1.0f / (1.0f + e);
      const float s = gv[t] >= 0.f ? inv : e * inv, t1 = gv[t] >= 0.f ? e * inv : inv;   // sigmoid(g), 1 - sigmoid(g)
      du[t] = yv[t] * (gv[t] * s);
      dg[t] = (yv[t] * uv[t]) * (s * fmaf(gv[t], t1, 1.0f));
    }
    *reinterpret_cast<float4*>(dgu + m * lddgu + c) = make_float4(dg[0], dg[1], dg[2], dg[3]);
    *reinterpret_cast<float4*>(dgu + m * lddgu + I + c) = make_float4(du[0], du[1], du[2], du[3]);
  }
}

// ------------------------------------------------------------------------------------------------ q / k norm + rotary embedding, backward
struct RopeBwdArgs {
  const float* qkv; int64_t ld;                  // the forward's input (pre-norm)
  const float *q_gamma, *k_gamma, *cos, *sin;
  const int32_t* positions;
  const float* dq; int64_t ldq;                  // gradient of the rotated q
  const float *dk, *dv; int64_t ldkv, kvbs;      // gradients of the cache rows, the cache's layout
  float* dqkv;                                   // [B Lq, ld]
  float* partial;                                // gain-gradient slabs: nslab_q x 128, then nslab_k x 128
  int rows, Lq, Hq, Hkv, Tmax;
  float eps;
};
// The rotation is orthogonal, so its backward is the transposed rotation of the lane-local pair (i, i + 64): a' = a cos + b sin, b' = b cos - a sin.  The returned pair
// is the gradient of the normed head; x0 / x1 / r are the head's pre-norm values and its rsqrt.
__device__ __forceinline__ void rope_bwd_head(const RopeBwdArgs& a, int row, int head, int lane, float& g0, float& g1, float& x0, float& x1, float& r) {
  const int b = row / a.Lq, pos = min(max(a.positions[row], 0), a.Tmax - 1);
  const float* src = a.qkv + (int64_t)row * a.ld + QD * head;
  x0 = src[lane]; x1 = src[lane + 64];
  const float* gsrc = head < a.Hq ? a.dq + (int64_t)row * a.ldq + QD * head : a.dk + (int64_t)b * a.kvbs + (int64_t)pos * a.ldkv + QD * (head - a.Hq);
  const float ya = gsrc[lane], yb = gsrc[lane + 64];
  const float cs = a.cos[(int64_t)pos * 64 + lane], sn = a.sin[(int64_t)pos * 64 + lane];
  g0 = fmaf(ya, cs, yb * sn);
  g1 = fmaf(yb, cs, -(ya * sn));
  r = __builtin_amdgcn_rsqf(wave_sum(fmaf(x0, x0, x1 * x1)) * (1.0f / QD) + a.eps);
}
__global__ __launch_bounds__(QTHREADS) void qk_norm_rope_bwd_kernel(RopeBwdArgs a) {
  const int heads = a.Hq + 2 * a.Hkv;
  const int64_t w = (int64_t)blockIdx.x * (QTHREADS / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= (int64_t)a.rows * heads) return;                        // wave-uniform
  const int row = (int)(w / heads), head = (int)(w - (int64_t)row * heads);
  float* dst = a.dqkv + (int64_t)row * a.ld + QD * head;
  if (head >= a.Hq + a.Hkv) {                                      // v: copied
    const int b = row / a.Lq, pos = min(max(a.positions[row], 0), a.Tmax - 1);
    const float* src = a.dv + (int64_t)b * a.kvbs + (int64_t)pos * a.ldkv + QD * (head - a.Hq - a.Hkv);
    dst[lane] = src[lane]; dst[lane + 64] = src[lane + 64];
    return;
  }
  float g0, g1, x0, x1, r;
  rope_bwd_head(a, row, head, lane, g0, g1, x0, x1, r);
  const float* g = head < a.Hq ? a.q_gamma : a.k_gamma;
  const float u0 = g[lane] * g0, u1 = g[lane + 64] * g1;
  const float coef = r * r * r * (wave_sum(fmaf(x0, u0, x1 * u1)) * (1.0f / QD));
  dst[lane] = fmaf(-x0, coef, r * u0);
  dst[lane + 64] = fmaf(-x1, coef, r * u1);
}
// Gain gradients dq_gamma[j] = sum over (row, q head) of g[j] x[j] r (likewise k): a workgroup owns a slab of kRopeSlab consecutive (row, head) pairs of one kind,
// wave w adds the pairs w, w + 4, ... in order, the four waves are added in wave order, the slabs in slab order by slab_reduce_kernel.
constexpr int kRopeSlab = 256;
__global__ __launch_bounds__(QTHREADS) void qk_gain_slab_kernel(RopeBwdArgs a, int nslab_q) {
  __shared__ float part[QTHREADS / 64][QD];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool is_q = (int)blockIdx.x < nslab_q;
  const int nh = is_q ? a.Hq : a.Hkv, slab = is_q ? blockIdx.x : blockIdx.x - nslab_q;
  const int64_t p0 = (int64_t)slab * kRopeSlab, p1 = min(p0 + kRopeSlab, (int64_t)a.rows * nh);
  float s0 = 0.f, s1 = 0.f;
  for (int64_t p = p0 + wave; p < p1; p += QTHREADS / 64) {        // wave-uniform trip count
    const int row = (int)(p / nh), head = (int)(p - (int64_t)row * nh) + (is_q ? 0 : a.Hq);
    float g0, g1, x0, x1, r;
    rope_bwd_head(a, row, head, lane, g0, g1, x0, x1, r);
    s0 = fmaf(g0, x0 * r, s0);
    s1 = fmaf(g1, x1 * r, s1);
  }
  part[wave][lane] = s0; part[wave][lane + 64] = s1;
  __syncthreads();
  if (threadIdx.x < QD) {
    const int t = threadIdx.x;
    a.partial[(int64_t)blockIdx.x * QD + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
  }
}
struct RopeWs { float* partial; int nslab_q, nslab_k; size_t bytes; };
RopeWs rope_bwd_layout(void* base, int64_t rows, int Hq, int Hkv) {
  Carver cv(base);
  const int nq = (int)((rows * Hq + kRopeSlab - 1) / kRopeSlab), nk = (int)((rows * Hkv + kRopeSlab - 1) / kRopeSlab);
  return {cv.take<float>((size_t)(nq + nk) * QD * 4), nq, nk, cv.bytes()};
}

}  // namespace

extern "C" int awt_op_rmsnorm(awt_ctx* c, const float* x, int64_t ldx, const float* gamma, float* y, int64_t ldy, int M, int d, float eps, void* stream) {
  AWT_REQUIRE(c && x && gamma && y, AWT_ERR_INVALID, "op_rmsnorm: null argument");
  AWT_REQUIRE(M > 0 && d > 0 && d % 4 == 0, AWT_ERR_INVALID, "op_rmsnorm: M must be positive and d a positive multiple of 4");
  AWT_REQUIRE(ldx >= d && ldy >= d && ldx % 4 == 0 && ldy % 4 == 0, AWT_ERR_INVALID, "op_rmsnorm: pitches must hold d columns and be multiples of 4");
  AWT_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(y), AWT_ERR_INVALID, "op_rmsnorm: tensors must be 16-byte aligned");
  AWT_REQUIRE(eps >= 0.f, AWT_ERR_INVALID, "op_rmsnorm: eps must not be negative");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_LAYERNORM, s);
  hipLaunchKernelGGL(rmsnorm_kernel, dim3((M + 3) / 4), dim3(QTHREADS), 0, s, x, ldx, gamma, y, ldy, M, d, eps);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" int awt_op_qk_norm_rope(awt_ctx* c, const float* qkv, int64_t ld, const float* q_gamma, const float* k_gamma, const float* cos, const float* sin,
                                   const int32_t* positions, float* q_out, int64_t ldq, float* k_cache, float* v_cache, int64_t ldkv, int64_t kv_batch_stride,
                                   int B, int Lq, int Hq, int Hkv, float eps, void* stream) {
  AWT_REQUIRE(c && qkv && q_gamma && k_gamma && cos && sin && positions && q_out && k_cache && v_cache, AWT_ERR_INVALID, "op_qk_norm_rope: null argument");
  AWT_REQUIRE(B > 0 && Lq > 0 && Hq > 0 && Hkv > 0, AWT_ERR_INVALID, "op_qk_norm_rope: B, Lq, Hq and Hkv must be positive");
  AWT_REQUIRE((int64_t)B * Lq < (1ll << 31) / (Hq + 2 * Hkv), AWT_ERR_INVALID, "op_qk_norm_rope: too many (row, head) pairs");
  AWT_REQUIRE(ld >= (int64_t)(Hq + 2 * Hkv) * QD && ldq >= (int64_t)Hq * QD && ldkv >= (int64_t)Hkv * QD, AWT_ERR_INVALID,
              "op_qk_norm_rope: ld must hold (Hq + 2 Hkv) * 128 columns, ldq Hq * 128, ldkv Hkv * 128 (head_dim is 128 in this operator)");
  AWT_REQUIRE(kv_batch_stride >= ldkv, AWT_ERR_INVALID, "op_qk_norm_rope: kv_batch_stride must hold at least one cache row");
  AWT_REQUIRE(eps >= 0.f, AWT_ERR_INVALID, "op_qk_norm_rope: eps must not be negative");
  RopeArgs a{};
  a.qkv = qkv; a.ld = ld; a.q_gamma = q_gamma; a.k_gamma = k_gamma; a.cos = cos; a.sin = sin; a.positions = positions; a.q_out = q_out; a.ldq = ldq;
  a.k_cache = k_cache; a.v_cache = v_cache; a.ldkv = ldkv; a.kvbs = kv_batch_stride;
  a.rows = B * Lq; a.Lq = Lq; a.Hq = Hq; a.Hkv = Hkv; a.eps = eps;
  a.Tmax = (int)std::min<int64_t>((kv_batch_stride - (int64_t)Hkv * QD) / ldkv + 1, 1ll << 30);   // cache rows of one batch that lie inside its stride
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_OTHER, s);
  const int64_t waves = (int64_t)a.rows * (Hq + 2 * Hkv);
  hipLaunchKernelGGL(qk_norm_rope_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(QTHREADS), 0, s, a);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" int awt_op_silu_mul(awt_ctx* c, const float* gu, int64_t ld, float* y, int64_t ldy, int M, int I, void* stream) {
  AWT_REQUIRE(c && gu && y, AWT_ERR_INVALID, "op_silu_mul: null argument");
  AWT_REQUIRE(M > 0 && I > 0 && I % 4 == 0, AWT_ERR_INVALID, "op_silu_mul: M must be positive and I a positive multiple of 4");
  AWT_REQUIRE(ld >= 2 * (int64_t)I && ldy >= I && ld % 4 == 0 && ldy % 4 == 0, AWT_ERR_INVALID,
              "op_silu_mul: ld must hold 2 I columns, ldy I, and both be multiples of 4");
  AWT_REQUIRE(aligned16(gu) && aligned16(y), AWT_ERR_INVALID, "op_silu_mul: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_OTHER, s);
  const int64_t n = (int64_t)M * (I / 4);
  const unsigned blocks = (unsigned)std::min<int64_t>((n + QTHREADS - 1) / QTHREADS, 256 * 32);
  hipLaunchKernelGGL(silu_mul_kernel, dim3(blocks), dim3(QTHREADS), 0, s, gu, ld, y, ldy, M, I);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

// ------------------------------------------------------------------------------------------------ backward entry points
extern "C" int awt_op_rmsnorm_backward(awt_ctx* c, const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma, const float* dres, float* dx,
                                       int64_t lddx, int M, int d, float eps, void* stream) {
  AWT_REQUIRE(c && dy && x && gamma && dx, AWT_ERR_INVALID, "op_rmsnorm_backward: null argument");
  AWT_REQUIRE(M > 0 && d > 0 && d % 4 == 0, AWT_ERR_INVALID, "op_rmsnorm_backward: M must be positive and d a positive multiple of 4");
  AWT_REQUIRE(lddy >= d && ldx >= d && lddx >= d && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0, AWT_ERR_INVALID,
              "op_rmsnorm_backward: pitches must hold d columns and be multiples of 4");
  AWT_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(gamma) && aligned16(dres) && aligned16(dx), AWT_ERR_INVALID,
              "op_rmsnorm_backward: tensors must be 16-byte aligned");
  AWT_REQUIRE(eps >= 0.f, AWT_ERR_INVALID, "op_rmsnorm_backward: eps must not be negative");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_LAYERNORM, s);
  hipLaunchKernelGGL(rmsnorm_bwd_kernel, dim3((M + 3) / 4), dim3(QTHREADS), 0, s, dy, lddy, x, ldx, gamma, dres, dx, lddx, M, d, eps);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" size_t awt_op_rmsnorm_param_grad_workspace_bytes(int M, int d) {
  if (M <= 0 || d <= 0) return 0;
  return gain_layout(nullptr, M, d).bytes;
}

extern "C" int awt_op_rmsnorm_param_grad(awt_ctx* c, const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dgamma, int M, int d, float eps,
                                         void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && dy && x && dgamma && workspace, AWT_ERR_INVALID, "op_rmsnorm_param_grad: null argument");
  AWT_REQUIRE(M > 0 && d > 0 && d % 4 == 0, AWT_ERR_INVALID, "op_rmsnorm_param_grad: M must be positive and d a positive multiple of 4");
  AWT_REQUIRE(lddy >= d && ldx >= d && lddy % 4 == 0 && ldx % 4 == 0, AWT_ERR_INVALID, "op_rmsnorm_param_grad: pitches must hold d columns and be multiples of 4");
  AWT_REQUIRE(aligned16(dy) && aligned16(x) && ((uintptr_t)workspace & 255) == 0, AWT_ERR_INVALID,
              "op_rmsnorm_param_grad: tensors must be 16-byte aligned, the workspace 256-byte aligned");
  AWT_REQUIRE(eps >= 0.f, AWT_ERR_INVALID, "op_rmsnorm_param_grad: eps must not be negative");
  AWT_REQUIRE(ws_bytes >= gain_layout(nullptr, M, d).bytes, AWT_ERR_WORKSPACE, "op_rmsnorm_param_grad: workspace too small");
  const int nslab = (M + kGainSlab - 1) / kGainSlab, gx = (d + QTHREADS - 1) / QTHREADS;
  AWT_REQUIRE(nslab <= 65535, AWT_ERR_INVALID, "op_rmsnorm_param_grad: too many rows");
  const GainWs ws = gain_layout(workspace, M, d);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_LAYERNORM, s);
  hipLaunchKernelGGL(rms_rstd_kernel, dim3((M + 3) / 4), dim3(QTHREADS), 0, s, x, ldx, ws.rstd, M, d, eps);
  hipLaunchKernelGGL(rms_gain_slab_kernel, dim3(gx, nslab), dim3(QTHREADS), 0, s, dy, lddy, x, ldx, ws.rstd, ws.partial, M, d);
  hipLaunchKernelGGL(slab_reduce_kernel, dim3(gx), dim3(QTHREADS), 0, s, ws.partial, nslab, d, dgamma);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" int awt_op_silu_mul_backward(awt_ctx* c, const float* gu, int64_t ld, const float* dy, int64_t lddy, float* dgu, int64_t lddgu, int M, int I, void* stream) {
  AWT_REQUIRE(c && gu && dy && dgu, AWT_ERR_INVALID, "op_silu_mul_backward: null argument");
  AWT_REQUIRE(M > 0 && I > 0 && I % 4 == 0, AWT_ERR_INVALID, "op_silu_mul_backward: M must be positive and I a positive multiple of 4");
  AWT_REQUIRE(ld >= 2 * (int64_t)I && lddgu >= 2 * (int64_t)I && lddy >= I && ld % 4 == 0 && lddgu % 4 == 0 && lddy % 4 == 0, AWT_ERR_INVALID,
              "op_silu_mul_backward: ld and lddgu must hold 2 I columns, lddy I, and all be multiples of 4");
  AWT_REQUIRE(aligned16(gu) && aligned16(dy) && aligned16(dgu), AWT_ERR_INVALID, "op_silu_mul_backward: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_OTHER, s);
  const int64_t n = (int64_t)M * (I / 4);
  const unsigned blocks = (unsigned)std::min<int64_t>((n + QTHREADS - 1) / QTHREADS, 256 * 32);
  hipLaunchKernelGGL(silu_mul_bwd_kernel, dim3(blocks), dim3(QTHREADS), 0, s, gu, ld, dy, lddy, dgu, lddgu, M, I);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" size_t awt_op_qk_norm_rope_backward_workspace_bytes(int B, int Lq, int Hq, int Hkv) {
  if (B <= 0 || Lq <= 0 || Hq <= 0 || Hkv <= 0) return 0;
  return rope_bwd_layout(nullptr, (int64_t)B * Lq, Hq, Hkv).bytes;
}

extern "C" int awt_op_qk_norm_rope_backward(awt_ctx* c, const float* qkv, int64_t ld, const float* q_gamma, const float* k_gamma, const float* cos, const float* sin,
                                            const int32_t* positions, const float* dq, int64_t ldq, const float* dk, const float* dv, int64_t ldkv,
                                            int64_t kv_batch_stride, float* dqkv, float* dq_gamma, float* dk_gamma, int B, int Lq, int Hq, int Hkv, float eps,
                                            void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && qkv && q_gamma && k_gamma && cos && sin && positions && dq && dk && dv && dqkv, AWT_ERR_INVALID, "op_qk_norm_rope_backward: null argument");
  AWT_REQUIRE(B > 0 && Lq > 0 && Hq > 0 && Hkv > 0, AWT_ERR_INVALID, "op_qk_norm_rope_backward: B, Lq, Hq and Hkv must be positive");
  AWT_REQUIRE((int64_t)B * Lq < (1ll << 31) / (Hq + 2 * Hkv), AWT_ERR_INVALID, "op_qk_norm_rope_backward: too many (row, head) pairs");
  AWT_REQUIRE(ld >= (int64_t)(Hq + 2 * Hkv) * QD && ldq >= (int64_t)Hq * QD && ldkv >= (int64_t)Hkv * QD, AWT_ERR_INVALID,
              "op_qk_norm_rope_backward: ld must hold (Hq + 2 Hkv) * 128 columns, ldq Hq * 128, ldkv Hkv * 128 (head_dim is 128 in this operator)");
  AWT_REQUIRE(kv_batch_stride >= ldkv, AWT_ERR_INVALID, "op_qk_norm_rope_backward: kv_batch_stride must hold at least one cache row");
  AWT_REQUIRE(eps >= 0.f, AWT_ERR_INVALID, "op_qk_norm_rope_backward: eps must not be negative");
  const bool gains = dq_gamma || dk_gamma;
  AWT_REQUIRE(!gains || (dq_gamma && dk_gamma && workspace && ((uintptr_t)workspace & 255) == 0), AWT_ERR_INVALID,
              "op_qk_norm_rope_backward: the gain gradients come as a pair and need a 256-byte aligned workspace");
  AWT_REQUIRE(!gains || ws_bytes >= rope_bwd_layout(nullptr, (int64_t)B * Lq, Hq, Hkv).bytes, AWT_ERR_WORKSPACE, "op_qk_norm_rope_backward: workspace too small");
  RopeBwdArgs a{};
  a.qkv = qkv; a.ld = ld; a.q_gamma = q_gamma; a.k_gamma = k_gamma; a.cos = cos; a.sin = sin; a.positions = positions; a.dq = dq; a.ldq = ldq;
  a.dk = dk; a.dv = dv; a.ldkv = ldkv; a.kvbs = kv_batch_stride; a.dqkv = dqkv;
  a.rows = B * Lq; a.Lq = Lq; a.Hq = Hq; a.Hkv = Hkv; a.eps = eps;
  a.Tmax = (int)std::min<int64_t>((kv_batch_stride - (int64_t)Hkv * QD) / ldkv + 1, 1ll << 30);   // as in the forward
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_OTHER, s);
  const int64_t waves = (int64_t)a.rows * (Hq + 2 * Hkv);
  hipLaunchKernelGGL(qk_norm_rope_bwd_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(QTHREADS), 0, s, a);
  if (gains) {
    const RopeWs ws = rope_bwd_layout(workspace, a.rows, Hq, Hkv);
    a.partial = ws.partial;
    hipLaunchKernelGGL(qk_gain_slab_kernel, dim3(ws.nslab_q + ws.nslab_k), dim3(QTHREADS), 0, s, a, ws.nslab_q);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(1), dim3(QTHREADS), 0, s, ws.partial, ws.nslab_q, QD, dq_gamma);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(1), dim3(QTHREADS), 0, s, ws.partial + (size_t)ws.nslab_q * QD, ws.nslab_k, QD, dk_gamma);
  }
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}
