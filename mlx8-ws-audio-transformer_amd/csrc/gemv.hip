// awt_linear_decode: the weight-streaming product of incremental decoding, y [M, Np] = x [M, K] W^T + bias (+ resid) for 1 <= M <= 8 rows, gfx950.
//
// At M <= 8 a linear layer is its weight read once: the 64-row-tile GEMM launches Np / 128 workgroups that each walk their whole K alone, with a plane-split
// launch in front (5.1 of a token's 6.5 ms).  This kernel reads the planes the `awt_weight` handle already owns -- w_frag_index order,
// one coalesced 1 KB block per (16-row n-tile, 32-deep k-step), 16 bytes per lane, which IS the B operand of v_mfma_f32_16x16x32_bf16 -- straight into
// registers with nontemporal loads, and forms the A operand itself: a lane with (lane & 15) < M loads its 8 consecutive fp32 values of x per k-step and
// splits them as split_planes_kernel does (split_bf16: hi = rne(x), lo = rne(x - hi)); lanes of rows >= M supply zeros and load nothing.  The products are
// the GEMM's: a_hi w_hi + a_hi w_lo + a_lo w_hi (PREC_BF16X3) or a_hi w_hi (PREC_BF16), accumulated in fp32.
//
// Decomposition (gemv_plan, from Np and K alone, never from M): a workgroup owns TT consecutive n-tiles and all of K; its waves take contiguous slices of
// `nk` k-steps each and walk them in chunks of KU k-steps x TT tiles, every load of a chunk issued before its first product.  Each wave leaves its partial
// 16 x 16 tiles (rows 0 .. 7: lanes 0 .. 31) in LDS; after ONE barrier the first 32 TT threads sum them in wave order 0, 1, ..., add bias and resid and store
// the M live rows.  A wave whose slice is empty contributes zeros and reaches the barrier like the others.  There is no communication between workgroups:
// no split-K across them, no counters, no atomics.  Hence the result is bit-reproducible, and row m of an M-row call is bit-identical to the M = 1 call on
// that row: an MFMA output element depends on its own A row only, and the order over K depends on (Np, K, precision) only.
#include <algorithm>
#include "common.h"

namespace {

struct GemvArgs {
  const bf16_t* w_hi; const bf16_t* w_lo;   // [Np, K] fragment-major planes (w_lo unused with one product)
  const float* bias;                        // [Np] or null
  const float* x; const float* resid; float* y;
  int M, K, Np, ksteps, nk;                 // ksteps = K / 32; nk = k-steps per wave
};

constexpr int kGemvMaxWaves = 16;

// PREC: PREC_BF16 | PREC_BF16X3.  Grid: Np / (16 TT) workgroups of `waves` x 64 threads; dynamic LDS: waves x TT x 512 bytes.
template <int PREC, int TT, int KU>
__global__ __launch_bounds__(kGemvMaxWaves * AWT_WAVE) void gemv_decode_kernel(const GemvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char gemv_smem[];
  f32x4* part = reinterpret_cast<f32x4*>(gemv_smem);                  // [wave][tile][lane < 32]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), waves = blockDim.x >> 6;   // wave in an SGPR: the slice loop is scalar
  const int row = lane & 15, kq = lane >> 4;                          // A fragment: x[row][32 ks + 8 kq + 0..7]
  const bool live = row < a.M;
  const int k0 = wave * a.nk, k1 = min(a.ksteps, k0 + a.nk);          // this wave's k-steps [k0, k1); empty when k0 >= ksteps
  const float* xr = a.x + (int64_t)row * a.K + 8 * kq;                // dereferenced by live lanes only
  const int64_t tile0 = (int64_t)blockIdx.x * TT;
  const char* whi = reinterpret_cast<const char*>(a.w_hi) + tile0 * a.ksteps * 1024 + lane * 16;
  const char* wlo = reinterpret_cast<const char*>(a.w_lo) + tile0 * a.ksteps * 1024 + lane * 16;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = zero4;

  for (int kb = k0; kb < k1; kb += KU) {
    // a chunk's k-steps past the slice (a slice that is no multiple of KU: K / 32 is not) repeat its last one, an address inside the matrix, and meet a zero
    // A operand below: loads and products stay unconditional, so that every load of the chunk is in flight before the first product waits
    int ks[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) ks[u] = min(kb + u, k1 - 1);
    float4 xa[KU][2];
#pragma unroll
    for (int u = 0; u < KU; ++u) xa[u][0] = xa[u][1] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        xa[u][0] = *reinterpret_cast<const float4*>(xr + 32 * ks[u]);
        xa[u][1] = *reinterpret_cast<const float4*>(xr + 32 * ks[u] + 4);
      }
    }
    bf16x8 wh[KU][TT], wl[KU][TT];
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const int64_t off = ((int64_t)t * a.ksteps + ks[u]) * 1024;
        wh[u][t] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(whi + off));
        if constexpr (PREC == PREC_BF16X3) wl[u][t] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wlo + off));
      }
    __builtin_amdgcn_sched_barrier(0);                                // left alone, hipcc sinks most of the chunk's loads below the first products: 2 in flight, not 8
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const float v[8] = {xa[u][0].x, xa[u][0].y, xa[u][0].z, xa[u][0].w, xa[u][1].x, xa[u][1].y, xa[u][1].z, xa[u][1].w};
      bf16x8 ah, al;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bf16_t h, l;
        split_bf16(v[j], h, l);
        const bool past = kb + u >= k1;                               // wave-uniform
        ah[j] = past ? (short)0 : (short)h; al[j] = past ? (short)0 : (short)l;
      }
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        acc[t] = mfma16<false>(ah, wh[u][t], acc[t]);
        if constexpr (PREC == PREC_BF16X3) {
          acc[t] = mfma16<false>(ah, wl[u][t], acc[t]);
          acc[t] = mfma16<false>(al, wh[u][t], acc[t]);
        }
      }
    }
  }

  // C fragment: column n = lane & 15, rows 4 (lane >> 4) + 0..3 -- rows 0 .. 7 live in lanes 0 .. 31
  if (lane < 32) {
#pragma unroll
    for (int t = 0; t < TT; ++t) part[(wave * TT + t) * 32 + lane] = acc[t];
  }
  __syncthreads();
  if (threadIdx.x < TT * 32) {
    const int t = threadIdx.x >> 5, slot = threadIdx.x & 31;
    f32x4 sum = part[t * 32 + slot];
    for (int w = 1; w < waves; ++w) sum += part[(w * TT + t) * 32 + slot];   // fixed order
    const int n = (int)(tile0 + t) * 16 + (slot & 15), m0 = (slot >> 4) * 4;
    const float b = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + r;
      if (m < a.M) {
        const int64_t o = (int64_t)m * a.Np + n;
        float v = sum[r] + b;
        if (a.resid) v += a.resid[o];
        a.y[o] = v;
      }
    }
  }
}

// Workgroup shape from Np and K alone.  Tiles per workgroup: 1 up to 2048 n-tiles (the model's layers: 64 .. 384 workgroups), 4 beyond (lm_head: 9 496
// n-tiles -> 2 374 workgroups), so that a chunk is KU x TT = 4 weight blocks per plane either way.  K-steps per wave: the least multiple of 4 (a whole
// number of the narrow form's chunks) that covers K with at most 16 waves; waves: what that takes, at least 4 -- K = 1024 -> 8 waves x 4 k-steps,
// K = 2048 -> 16 x 4, K = 3072 -> 12 x 8, K = 192 -> 4 waves holding 4, 2, 0, 0 k-steps, K = 64 -> 2, 0, 0, 0.
struct GemvPlan { int tt, waves, nk; };
GemvPlan gemv_plan(int Np, int K) {
  const int ntiles = Np / 16, ksteps = K / 32;
  GemvPlan p;
  p.tt = ntiles > 2048 ? 4 : 1;
  p.nk = 4 * ((ksteps + 4 * kGemvMaxWaves - 1) / (4 * kGemvMaxWaves));
  p.waves = std::max(4, (ksteps + p.nk - 1) / p.nk);
  return p;
}

template <int PREC>
int launch_gemv(const GemvPlan& p, const GemvArgs& a, hipStream_t s) {
  const dim3 grid(a.Np / (16 * p.tt)), block(p.waves * AWT_WAVE);
  const int lds = p.waves * p.tt * 32 * (int)sizeof(f32x4);
  if (p.tt == 1) return launch_kernel<gemv_decode_kernel<PREC, 1, 4>>(grid, block, lds, s, a);
  return launch_kernel<gemv_decode_kernel<PREC, 4, 1>>(grid, block, lds, s, a);
}

}  // namespace

extern "C" int awt_linear_decode(awt_ctx* c, const awt_weight* w, const float* x, const float* resid, float* y, int M, void* stream) {
  AWT_REQUIRE(c && w && x && y, AWT_ERR_INVALID, "linear_decode: null argument");
  AWT_REQUIRE(M >= 1 && M <= 8, AWT_ERR_INVALID, "linear_decode: M must be in [1, 8] (awt_linear_forward takes any M)");
  AWT_REQUIRE(w->prec == PREC_BF16 || w->prec == PREC_BF16X3, AWT_ERR_INVALID, "linear_decode: the weight's precision must be 1 (bf16) or 3 (bf16x3)");
  AWT_REQUIRE(w->Np % 64 == 0 && w->K % 32 == 0, AWT_ERR_INVALID, "linear_decode: the weight's padded rows must be a multiple of 64 and K of 32");
  AWT_REQUIRE(((uintptr_t)x & 15) == 0, AWT_ERR_INVALID, "linear_decode: x must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const GemvPlan p = gemv_plan(w->Np, w->K);
  GemvArgs a{w->hi, w->prec == PREC_BF16X3 ? w->lo : w->hi, w->bias, x, resid, y, M, w->K, w->Np, w->K / 32, p.nk};
  ProfScope prof(c, AWT_PROF_GEMM, s, 2.0 * (double)M * (double)w->N * (double)w->K);
  return w->prec == PREC_BF16X3 ? launch_gemv<PREC_BF16X3>(p, a, s) : launch_gemv<PREC_BF16>(p, a, s);
}
