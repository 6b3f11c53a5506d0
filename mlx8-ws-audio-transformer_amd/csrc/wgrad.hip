// Weight-gradient GEMM of the full-parameter encoder backward:  dW[n, k] = scale * sum_m dY[m, ycol + n] X[rowmap(m), xcol + k]
//
// Both operands are the library's ROW-MAJOR bf16 plane pairs (hi, lo), exactly as the forward-for-training and the backward pass leave
// them; the contraction index m is the ROW index of both.  An MFMA wants the contraction index inside a lane's fragment, i.e. both
// operands transposed.  Nothing is transposed in memory: a [32 rows of m][128 columns] tile of each plane is staged in LDS as it comes
// from HBM (16-byte chunks, coalesced) and the fragments are fetched with gfx950's transposed LDS read ds_read_b64_tr_b16, which hands
// lane i of a 16-lane group column i of a 4-row x 16-column block.  For v_mfma_f32_32x32x16_bf16 (lane l, r = l & 31, h = l >> 5 holds
// A[r][8 h + j] and B[8 h + j][r], j < 8) with A = dY^T and B = X both fragments are "column r of rows 8 h .. 8 h + 7 of the tile": two
// transposed reads (rows 8 h + 0..3 and 8 h + 4..7) in which 16-lane group g takes columns 16 (g & 1) .. + 15 and rows 8 (g >> 1) ...
//
// LDS image: plain rows of 128 elements (256 bytes) at a pitch of 320 bytes.  Bank rule (64 banks of 4 bytes, conflicts counted per
// 32-lane half): one half reads 4 consecutive rows x 32 columns = 4 x 64 bytes; with 320 = 5 x 64 the rows start 80 dwords = 16 banks
// (mod 64) apart, so the four 16-bank runs tile the 64 banks: conflict-free.  Every lane address is a multiple of 8 bytes (pitch, 32-column
// subtile = 64 bytes, 4 columns = 8 bytes).  EXEC is all ones at every transposed read: the tile is padded with zeros (rows beyond the slab or
// M, columns beyond N / K, row-map rows outside the clip) instead of masking lanes, and zero rows add nothing to the sum.
//
// Grid: the output has few tiles (d = 768: 36 tiles of 128 x 128 on 256 CUs), so M is cut into slabs: grid = tiles x slabs, each workgroup
// writes its fp32 partial tile to workspace, and a second launch adds the slabs in ascending order and applies scale / accumulate.  The slab count
// is a function of (M, N, K) only and there are no atomics: results are bit-reproducible.  Products per fragment pair follow the backward's
// `gterms`: one bf16 product, or hi lo + lo hi + hi hi.
#include <algorithm>

#include "common.h"
#include "wgrad.h"

namespace {

constexpr int BN = 128, BKC = 128, BM = 32;       // output tile [BN x BKC], rows of m per staged tile
constexpr int PITCH = 320;                        // bytes per LDS row (256 + 64: see the bank rule above)
constexpr int PLANE = BM * PITCH;                 // 10240 bytes per plane tile
constexpr int kTargetGroups = 512;                // two workgroups per CU

struct WgradArgs {
  const bf16_t *y_hi, *y_lo; int64_t ldy; int ycol, N;
  const bf16_t *x_hi, *x_lo; int64_t ldx; int xcol, K;
  int M, slab_rows;
  int rows_out, rows_in, row_mul, row_add;        // X row of contraction row m (common.h row_map_source; outside [0, rows_in): zero)
  float* partial;                                 // [slabs][N][K]
};

__device__ __forceinline__ bf16x4 tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)p);
}
__device__ __forceinline__ bf16x8 tr_frag(const char* p) {   // rows r0 .. r0 + 3 and r0 + 4 .. r0 + 7 of the lane's column
  const bf16x4 a = tr_read(p), b = tr_read(p + 4 * PITCH);
  return (bf16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// one 16-byte chunk of row m of each operand plane (zeros beyond the slab, beyond the operand's width, and for row-map rows outside the clip)
template <int NP>
__device__ __forceinline__ void load_row(const WgradArgs& g, int m, int m_end, bool ycol_ok, bool xcol_ok, int64_t ycoff, int64_t xcoff, uint4& yh, uint4& yl,
                                         uint4& xh, uint4& xl) {
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  const bool mok = m < m_end, yok = mok && ycol_ok;
  const int64_t yo = (int64_t)m * g.ldy + ycoff;
  yh = z;
  if (yok) yh = *reinterpret_cast<const uint4*>(g.y_hi + yo);
  if constexpr (NP == 2) { yl = z; if (yok) yl = *reinterpret_cast<const uint4*>(g.y_lo + yo); }
  int64_t xrow;
  const bool xin = row_map_source(m, g.rows_out, g.rows_in, g.row_mul, g.row_add, xrow);
  const bool xok = mok && xcol_ok && xin;
  const int64_t xo = xrow * g.ldx + xcoff;
  xh = z;
  if (xok) xh = *reinterpret_cast<const uint4*>(g.x_hi + xo);
  if constexpr (NP == 2) { xl = z; if (xok) xl = *reinterpret_cast<const uint4*>(g.x_lo + xo); }
}

template <int TERMS>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs g) {
  constexpr int NP = TERMS == 3 ? 2 : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];     // [Y hi | Y lo | X hi | X lo] plane tiles
  char* const ys = smem;
  char* const xs = smem + NP * PLANE;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int k0 = blockIdx.x * BKC, n0 = blockIdx.y * BN;
  const int m_begin = blockIdx.z * g.slab_rows, m_end = min(g.M, m_begin + g.slab_rows);

  // staging: a plane tile is 32 rows x 16 chunks of 16 bytes; thread t copies chunks t and t + 256 (rows t / 16 and t / 16 + 16)
  const int srow = tid >> 4, sch = tid & 15;
  const bool ycol_ok = n0 + sch * 8 < g.N, xcol_ok = k0 + sch * 8 < g.K;
  const int64_t ycoff = g.ycol + n0 + sch * 8, xcoff = g.xcol + k0 + sch * 8;
  // the two rows a thread stages, as named registers (arrays indexed through a helper end up in scratch memory)
  uint4 yh0, yl0, xh0, xl0, yh1, yl1, xh1, xl1;
  yl0 = xl0 = yl1 = xl1 = make_uint4(0u, 0u, 0u, 0u);
  auto load = [&](int m0) __attribute__((always_inline)) {
    load_row<NP>(g, m0 + srow, m_end, ycol_ok, xcol_ok, ycoff, xcoff, yh0, yl0, xh0, xl0);
    load_row<NP>(g, m0 + srow + 16, m_end, ycol_ok, xcol_ok, ycoff, xcoff, yh1, yl1, xh1, xl1);
  };
  auto stash = [&]() __attribute__((always_inline)) {
    const int off0 = srow * PITCH + sch * 16, off1 = off0 + 16 * PITCH;
    *reinterpret_cast<uint4*>(ys + off0) = yh0; *reinterpret_cast<uint4*>(xs + off0) = xh0;
    *reinterpret_cast<uint4*>(ys + off1) = yh1; *reinterpret_cast<uint4*>(xs + off1) = xh1;
    if constexpr (NP == 2) {
      *reinterpret_cast<uint4*>(ys + PLANE + off0) = yl0; *reinterpret_cast<uint4*>(xs + PLANE + off0) = xl0;
      *reinterpret_cast<uint4*>(ys + PLANE + off1) = yl1; *reinterpret_cast<uint4*>(xs + PLANE + off1) = xl1;
    }
  };

  // fragment addresses: wave (wn, wk) owns the 64 x 64 quadrant at (64 wn, 64 wk) of the tile = 2 x 2 MFMA tiles of 32 x 32.
  // Lane 16 g + 4 q + p supplies row 8 (g >> 1) + q, columns 16 (g & 1) + 4 p .. + 3 of the 32-column subtile (8 bytes).
  const int wn = wave >> 1, wk = wave & 1;
  const int grp16 = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
  const int foff = (8 * (grp16 >> 1) + q) * PITCH + (16 * (grp16 & 1) + 4 * p4) * 2;
  const char* const ya = ys + foff + wn * 128;     // 64 columns = 128 bytes
  const char* const xa = xs + foff + wk * 128;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[i][j][t] = 0.f;

  if (m_begin < m_end) load(m_begin);
  for (int m0 = m_begin; m0 < m_end; m0 += BM) {
    stash();
    __syncthreads();
    if (m0 + BM < m_end) load(m0 + BM);            // the next tile's global loads fly during this tile's MFMAs
#pragma unroll
    for (int ms = 0; ms < BM / 16; ++ms) {
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int o = ms * 16 * PITCH + i * 64;    // 16 rows down, 32 columns = 64 bytes across
        ah[i] = tr_frag(ya + o); bh[i] = tr_frag(xa + o);
        if constexpr (TERMS == 3) { al[i] = tr_frag(ya + PLANE + o); bl[i] = tr_frag(xa + PLANE + o); }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if constexpr (TERMS == 3) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
          }
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
  }

  // D[row = n][col = k]: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* const part = g.partial + (int64_t)blockIdx.z * g.N * g.K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + wk * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int n = n0 + wn * 64 + i * 32 + (t & 3) + 8 * (t >> 2) + 4 * (lane >> 5);
        if (n < g.N && k < g.K) part[(int64_t)n * g.K + k] = acc[i][j][t];
      }
    }
}

// out[n sn + k sk] (+)= scale * (slab 0 + slab 1 + ...): fixed order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int nslab, int N, int K, float scale, float* out,
                                                           int64_t sn, int64_t sk, int accumulate) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)N * K;
  if (e >= total) return;
  float a = 0.f;
  for (int s = 0; s < nslab; ++s) a += partial[(int64_t)s * total + e];
  const int n = (int)(e / K), k = (int)(e - (int64_t)n * K);
  float* dst = out + n * sn + k * sk;
  a *= scale;
  *dst = accumulate ? *dst + a : a;
}

// dy * gelu'(pre) as operand planes (conv2's pre-activation is recomputed in fp32 by the backward pass)
__global__ __launch_bounds__(256) void dgelu_planes_kernel(const float* __restrict__ dy, const float* __restrict__ pre, int64_t n4, bf16_t* hi, bf16_t* lo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const float4 g = reinterpret_cast<const float4*>(dy)[i], x = reinterpret_cast<const float4*>(pre)[i];
  const float gv[4] = {g.x, g.y, g.z, g.w}, xv[4] = {x.x, x.y, x.z, x.w};
  float v[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)   // d/dx gelu(x) = Phi(x) + x phi(x), as the GEMM's EPI_BF16_DGELU epilogue forms it
    v[t] = gv[t] * (0.5f * (1.0f + erf_fast(xv[t] * 0.70710678118654752440f)) + xv[t] * 0.39894228040143267794f * __expf(-0.5f * xv[t] * xv[t]));
  Act o; o.p16 = hi; o.lo16 = lo;
  store_act4<PREC_BF16X3>(o, i * 4, v);
}

// dst[n, c] = src[n, c, tap] of a Conv1d weight [N, C, 3]
__global__ __launch_bounds__(256) void conv_tap_kernel(const float* __restrict__ src, int64_t n, int tap, float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i * 3 + tap];
}

}  // namespace

int wgrad_slabs(int M, int N, int K, int* slab_rows) {
  const int64_t tiles = (int64_t)((N + BN - 1) / BN) * ((K + BKC - 1) / BKC);
  int64_t want = (kTargetGroups + tiles - 1) / tiles;
  want = std::max<int64_t>(1, std::min<int64_t>(want, (M + 255) / 256));     // a slab is at least 256 rows
  const int rows = (int)(((M + want - 1) / want + BM - 1) / BM * BM);
  if (slab_rows) *slab_rows = rows;
  return (M + rows - 1) / rows;
}
size_t wgrad_partial_bytes(int M, int N, int K) { return (size_t)wgrad_slabs(M, N, K, nullptr) * (size_t)N * (size_t)K * 4; }

int launch_wgrad(awt_ctx* c, const WgradOperand& y, int N, const WgradOperand& x, int K, int M, const WgradRowMap* map, int terms, float scale,
                 float* out, int64_t sn, int64_t sk, int accumulate, float* partial, size_t partial_bytes, hipStream_t s) {
  AWT_REQUIRE(c && y.hi && x.hi && out && partial && M > 0 && N > 0 && K > 0, AWT_ERR_INVALID, "weight_grad: null or empty argument");
  AWT_REQUIRE(terms == 1 || (terms == 3 && y.lo && x.lo), AWT_ERR_INVALID, "weight_grad: terms must be 1, or 3 with both lo planes");
  AWT_REQUIRE(N % 8 == 0 && K % 8 == 0 && y.ld % 8 == 0 && x.ld % 8 == 0 && y.col % 8 == 0 && x.col % 8 == 0 && y.col >= 0 && x.col >= 0 &&
                  y.col + N <= y.ld && x.col + K <= x.ld, AWT_ERR_INVALID,
              "weight_grad: widths, pitches and column offsets must be multiples of 8 and the columns must lie inside their rows");
  AWT_REQUIRE(((uintptr_t)y.hi & 15) == 0 && ((uintptr_t)x.hi & 15) == 0 && ((uintptr_t)y.lo & 15) == 0 && ((uintptr_t)x.lo & 15) == 0, AWT_ERR_INVALID,
              "weight_grad: planes must be 16-byte aligned");
  AWT_REQUIRE(!map || (map->rows_out > 0 && map->rows_in > 0 && M % map->rows_out == 0), AWT_ERR_INVALID, "weight_grad: bad row map");
  AWT_REQUIRE(partial_bytes >= wgrad_partial_bytes(M, N, K), AWT_ERR_WORKSPACE, "weight_grad: workspace too small");
  WgradArgs a{};
  a.y_hi = y.hi; a.y_lo = y.lo; a.ldy = y.ld; a.ycol = y.col; a.N = N;
  a.x_hi = x.hi; a.x_lo = x.lo; a.ldx = x.ld; a.xcol = x.col; a.K = K;
  a.M = M; a.partial = partial;
  if (map) { a.rows_out = map->rows_out; a.rows_in = map->rows_in; a.row_mul = map->row_mul; a.row_add = map->row_add; }
  else { a.rows_out = M; a.rows_in = M; a.row_mul = 1; a.row_add = 0; }
  const int slabs = wgrad_slabs(M, N, K, &a.slab_rows);
  const dim3 grid((K + BKC - 1) / BKC, (N + BN - 1) / BN, slabs);
  ProfScope prof(c, AWT_PROF_WGRAD, s, 2.0 * (double)M * (double)N * (double)K);
  int rc = terms == 3 ? launch_kernel<wgrad_kernel<3>>(grid, dim3(256), 4 * PLANE, s, a) : launch_kernel<wgrad_kernel<1>>(grid, dim3(256), 2 * PLANE, s, a);
  if (rc) return rc;
  const int64_t total = (int64_t)N * K;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)partial, slabs, N, K, scale, out, sn, sk, accumulate);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

int launch_dgelu_planes(awt_ctx* c, const float* dy, const float* pre, int64_t n, const PlanePair& out, hipStream_t s) {
  AWT_REQUIRE(c && dy && pre && out.hi && n > 0 && n % 4 == 0, AWT_ERR_INVALID, "dgelu_planes: bad argument");
  hipLaunchKernelGGL(dgelu_planes_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, dy, pre, n / 4, out.hi, out.lo);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

int launch_conv_tap(awt_ctx* c, const float* src, int N, int C, int tap, float* dst, hipStream_t s) {
  AWT_REQUIRE(c && src && dst && N > 0 && C > 0 && tap >= 0 && tap < 3, AWT_ERR_INVALID, "conv_tap: bad argument");
  const int64_t n = (int64_t)N * C;
  hipLaunchKernelGGL(conv_tap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, n, tap, dst);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

// ------------------------------------------------------------------------------------------------ single-operator entry (include/awt.h)
namespace {
// awt_op_weight_grad's workspace: the split-bf16 planes of dy [M, ldy] and of x [rows_x, ldx], then the slab partials of the product
struct OpWgradWs { PlanePair y, x; float* partial; size_t partial_bytes, bytes; };
OpWgradWs op_wgrad_layout(void* base, int M, int rows_x, int ldy, int ldx, int N, int K) {
  const size_t pb = align_up(N > 0 && K > 0 ? wgrad_partial_bytes(M, N, K) : 0);     // an empty product: launch_wgrad refuses it
  Carver cv(base);
  return {take_planes(cv, (size_t)M * ldy), take_planes(cv, (size_t)rows_x * ldx), cv.take<float>(pb), pb, cv.bytes()};
}
}  // namespace
extern "C" size_t awt_op_weight_grad_workspace_bytes(int M, int rows_x, int ldy, int ldx, int N, int K) {
  if (M <= 0 || rows_x <= 0 || ldy <= 0 || ldx <= 0 || N <= 0 || K <= 0) return 0;
  return op_wgrad_layout(nullptr, M, rows_x, ldy, ldx, N, K).bytes;
}
extern "C" int awt_op_weight_grad(awt_ctx* c, const float* dy, int ldy, int ycol, int N, const float* x, int rows_x, int ldx, int xcol, int K, int M,
                                  int rows_out, int rows_in, int row_mul, int row_add, int terms, float scale, int accumulate, float* out,
                                  int64_t sn, int64_t sk, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && dy && x && out && workspace && M > 0 && rows_x > 0 && ldy > 0 && ldx > 0, AWT_ERR_INVALID, "op_weight_grad: null or empty argument");
  AWT_REQUIRE(terms == 1 || terms == 3, AWT_ERR_INVALID, "op_weight_grad: terms must be 1 (bf16) or 3 (bf16x3)");
  AWT_REQUIRE(((int64_t)M * ldy) % 4 == 0 && ((int64_t)rows_x * ldx) % 4 == 0, AWT_ERR_INVALID, "op_weight_grad: operand element counts must be multiples of 4");
  AWT_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)dy & 15) == 0 && ((uintptr_t)x & 15) == 0, AWT_ERR_INVALID,
              "op_weight_grad: workspace must be 256-byte aligned, tensors 16-byte aligned");
  const bool mapped = rows_out > 0;
  AWT_REQUIRE(mapped ? (rows_in > 0 && M % rows_out == 0 && (int64_t)(M / rows_out) * rows_in == rows_x) : rows_x == M, AWT_ERR_INVALID,
              "op_weight_grad: x must have M rows, or (M / rows_out) * rows_in rows under a row map");
  AWT_REQUIRE(ws_bytes >= awt_op_weight_grad_workspace_bytes(M, rows_x, ldy, ldx, N, K), AWT_ERR_WORKSPACE, "op_weight_grad: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const OpWgradWs w = op_wgrad_layout(workspace, M, rows_x, ldy, ldx, N, K);
  int rc = launch_split_f32(c, dy, (int64_t)M * ldy, 1.0f, w.y, s); if (rc) return rc;
  rc = launch_split_f32(c, x, (int64_t)rows_x * ldx, 1.0f, w.x, s); if (rc) return rc;
  const WgradOperand yo{w.y.hi, w.y.lo, ldy, ycol}, xo{w.x.hi, w.x.lo, ldx, xcol};
  const WgradRowMap map{rows_out, rows_in, row_mul, row_add};
  return launch_wgrad(c, yo, N, xo, K, M, mapped ? &map : nullptr, terms, scale, out, sn, sk, accumulate, w.partial, w.partial_bytes, s);
}
