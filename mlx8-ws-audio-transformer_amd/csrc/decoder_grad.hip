// Row kernels of the DECODER's parameter gradients (full-parameter fine-tuning, NativeWhisperDecoder train_base), gfx950.
//
// The decoder's weight gradients are products on the weight-gradient GEMM (wgrad.hip) and its LayerNorm gradients come from
// decoder_ops.hip; what is left are two HBM-bound reductions:
//  * awt_op_embed_backward: the backward of awt_op_embed -- a scatter-add of B L rows into the [vocab, d] token table (ids repeat: the
//    start token heads every clip, the pad token fills every short row) and into the position table;
//  * awt_op_column_sums_ld: bias gradients as column sums of a column window of a pitched matrix (the q / v blocks of the fused
//    [M, 3 d] gradient, fc1's 4 d columns, the value blocks of the [B S, 2 layers d] cross buffer).
// Both are deterministic: no atomics, every sum is formed in a fixed order, so two runs give the same bits.  Every lane moves 16 bytes per
// access (float4), neighbouring lanes neighbouring 16 bytes.
#include "common.h"

namespace {

constexpr int kEmbMaxVec = 2;             // float4 groups per thread: d <= 4 * 256 * kEmbMaxVec = 2048

__device__ __forceinline__ int64_t clamp_id(int64_t id, int vocab) { return id < 0 ? 0 : (id >= vocab ? vocab - 1 : id); }   // as embed_kernel reads
__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

// Workgroups 0 .. M - 1: workgroup m owns token row clamp(ids[m]) iff no earlier row has that id (otherwise it leaves: the owner sums this
// row too); it then adds dx[m'] over every m' >= m with the same id in ascending m' and adds the total to dtok[id].  One workgroup writes a
// table row, so rows are race-free; rows no id names are not touched.
// Workgroups M .. M + L - 1: workgroup M + l adds dx[b L + l] over b ascending to dpos[pos0 + l].
// The id scan walks ids in chunks of 256 (one id per thread); a wave's matches are a 64-bit ballot, parked in LDS so that all four waves walk
// the chunk's matches in ascending order.
__global__ __launch_bounds__(256) void embed_bwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dx, int M, int L, int d, int pos0,
                                                        int vocab, float* dtok, float* dpos) {
  __shared__ unsigned long long hit[4];
  const int tid = threadIdx.x, nv = d >> 2;
  float4 acc[kEmbMaxVec];
#pragma unroll
  for (int j = 0; j < kEmbMaxVec; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  auto add_row = [&](int row) __attribute__((always_inline)) {
    const float4* r = reinterpret_cast<const float4*>(dx + (int64_t)row * d);
#pragma unroll
    for (int j = 0; j < kEmbMaxVec; ++j) { const int i = tid + 256 * j; if (i < nv) add4(acc[j], r[i]); }
  };
  auto add_to = [&](float* dst) __attribute__((always_inline)) {
    float4* o = reinterpret_cast<float4*>(dst);
#pragma unroll
    for (int j = 0; j < kEmbMaxVec; ++j) { const int i = tid + 256 * j; if (i < nv) { float4 v = o[i]; add4(v, acc[j]); o[i] = v; } }
  };
  if ((int)blockIdx.x >= M) {                                      // position rows
    const int l = blockIdx.x - M;
    for (int row = l; row < M; row += L) add_row(row);
    add_to(dpos + (int64_t)(pos0 + l) * d);
    return;
  }
  const int m = blockIdx.x;
  const int64_t id = clamp_id(ids[m], vocab);
  for (int base = 0; base < m; base += 256) {                      // an earlier row with this id owns the table row
    const int r = base + tid;
    if (__syncthreads_or(r < m && clamp_id(ids[r], vocab) == id)) return;
  }
  for (int base = m & ~255; base < M; base += 256) {
    const int r = base + tid;
    const unsigned long long b = __builtin_amdgcn_ballot_w64(r >= m && r < M && clamp_id(ids[r], vocab) == id);
    if ((tid & 63) == 0) hit[tid >> 6] = b;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      unsigned long long bits = hit[w];                            // the same value in every thread: the loop is uniform
      while (bits) {
        const int t = __builtin_ctzll(bits);
        bits &= bits - 1;
        add_row(base + 64 * w + t);
      }
    }
    __syncthreads();
  }
  add_to(dtok + id * d);
}

// Column sums of the window [col, col + width) of a [M, ld] matrix.  A thread owns four consecutive columns (one float4 per row), a
// workgroup 1024 columns of one slab of kSumSlab rows, walked top to bottom; partial [slabs][width], added in slab order by the second kernel.
constexpr int kSumSlab = 256;
__global__ __launch_bounds__(256) void column_sums_ld_kernel(const float* __restrict__ a, int M, int64_t ld, int col, int width, float* __restrict__ partial) {
  const int c4 = blockIdx.x * 256 + threadIdx.x;
  if (c4 * 4 >= width) return;
  const int r0 = blockIdx.y * kSumSlab, r1 = min(M, r0 + kSumSlab);
  const float* p = a + (int64_t)r0 * ld + col + c4 * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r = r0; r < r1; ++r, p += ld) add4(s, *reinterpret_cast<const float4*>(p));
  reinterpret_cast<float4*>(partial + (int64_t)blockIdx.y * width)[c4] = s;
}
__global__ __launch_bounds__(256) void column_sums_ld_reduce_kernel(const float* __restrict__ partial, int nslab, int width, float* sums, int accumulate) {
  const int c4 = blockIdx.x * 256 + threadIdx.x;
  if (c4 * 4 >= width) return;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = 0; i < nslab; ++i) add4(s, reinterpret_cast<const float4*>(partial + (int64_t)i * width)[c4]);
  float4* o = reinterpret_cast<float4*>(sums) + c4;
  if (accumulate) { float4 v = *o; add4(v, s); s = v; }
  *o = s;
}

}  // namespace

extern "C" int awt_op_embed_backward(awt_ctx* c, const int64_t* ids, const float* dx, float* dtok, float* dpos, int M, int L, int d, int pos0,
                                     int vocab, void* stream) {
  AWT_REQUIRE(c && ids && dx && dtok && dpos && M > 0 && L > 0 && M % L == 0 && d > 0 && d % 4 == 0 && d <= 1024 * kEmbMaxVec && pos0 >= 0 && vocab > 0,
              AWT_ERR_INVALID, "op_embed_backward: bad argument (M a multiple of L, d a multiple of 4 and at most 2048)");
  AWT_REQUIRE((((uintptr_t)dx | (uintptr_t)dtok | (uintptr_t)dpos) & 15) == 0, AWT_ERR_INVALID, "op_embed_backward: tensors must be 16-byte aligned");
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(M + L), dim3(256), 0, (hipStream_t)stream, ids, dx, M, L, d, pos0, vocab, dtok, dpos);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" size_t awt_op_column_sums_ld_workspace_bytes(int M, int width) {
  if (M <= 0 || width <= 0) return 0;
  return (size_t)((M + kSumSlab - 1) / kSumSlab) * (size_t)width * 4;
}
extern "C" int awt_op_column_sums_ld(awt_ctx* c, const float* a, int64_t ld, int col, int width, float* sums, int M, int accumulate, void* workspace,
                                     size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && a && sums && workspace && M > 0 && width > 0 && col >= 0, AWT_ERR_INVALID, "op_column_sums_ld: null or empty argument");
  AWT_REQUIRE(width % 4 == 0 && col % 4 == 0 && ld % 4 == 0 && (int64_t)col + width <= ld, AWT_ERR_INVALID,
              "op_column_sums_ld: width, col and ld must be multiples of 4 and the window must lie inside a row");
  AWT_REQUIRE((((uintptr_t)a | (uintptr_t)sums | (uintptr_t)workspace) & 15) == 0, AWT_ERR_INVALID, "op_column_sums_ld: tensors must be 16-byte aligned");
  AWT_REQUIRE(ws_bytes >= awt_op_column_sums_ld_workspace_bytes(M, width), AWT_ERR_WORKSPACE, "op_column_sums_ld: workspace too small");
  const int nslab = (M + kSumSlab - 1) / kSumSlab, gx = (width / 4 + 255) / 256;
  AWT_REQUIRE(nslab <= 65535, AWT_ERR_INVALID, "op_column_sums_ld: too many rows");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(column_sums_ld_kernel, dim3(gx, nslab), dim3(256), 0, s, a, M, ld, col, width, (float*)workspace);
  hipLaunchKernelGGL(column_sums_ld_reduce_kernel, dim3(gx), dim3(256), 0, s, (const float*)workspace, nslab, width, sums, accumulate);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}
