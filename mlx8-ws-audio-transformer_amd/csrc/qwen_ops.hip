// The row operators of a Qwen3 decoder layer that the library did not have -- gfx950.  All fp32 in, fp32 out, on the caller's stream, HBM-bound.
//   awt_op_rmsnorm        y = gamma x rsqrt(mean(x^2) + eps)                      one wave per row, x read twice (the second time from cache)
//   awt_op_qk_norm_rope   per-head RMSNorm of q and k, rotary embedding, q to its own buffer, k and v into the decode cache: one wave per (row, head)
//   awt_op_silu_mul       y = silu(gate) * up over one [M, 2 I] gate | up GEMM output   16-byte accesses
// The causal attention of the layer is the CAUSAL variant of csrc/cross_attention.hip's forward.  (music2midi.Qwen3Decoder)
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
