// Token selection and beam cache reordering of `generate` (HF 5.15 `GenerationMixin._sample` / `_beam_search` with Whisper's suppress
// processors, and `WhisperGenerationMixin.detect_language`), gfx950.
//
// awt_op_select_tokens turns the decoder's last-position logits into the next tokens.  Per row (one hypothesis): log-softmax over all
// `vocab` columns (optional), banned columns set to -inf, the row's running beam score added; per clip (`beams` consecutive rows): the
// top k of the beams x vocab candidates, best first.  Greedy decoding is beams = 1, k = 1 without log-softmax: argmax after banning, ties
// to the lowest column, NaN first (torch.argmax).  Two launches, no atomics:
//  (1) select_partial_kernel: a workgroup per (row, column chunk) reads its chunk with float4 loads; each lane keeps an online
//      (max, sum exp) pair and a register top-KP list (KP = k rounded up to a power of two), merged across the 64 lanes and 4 waves through
//      LDS (pairwise sorted-list merges, fixed order); the chunk's pair and list go to the workspace;
//  (2) select_final_kernel: a workgroup per clip folds each row's chunk pairs into its log-sum-exp (chunk order), turns the chunk lists
//      into scores ((x - max) - log sum + beam score, torch's order of operations) and merges them the same way.
// The top k of a clip is among the top k of its rows' chunks: the scores are a monotone per-row shift of the banned logits.
//
// awt_op_kv_gather copies the self-attention cache rows parent[r] -> r ([layers, rows, Tmax, width], first T positions) into a second
// buffer in one launch: the per-step beam reorder (HF `_reorder_cache`) and the B -> B x num_beams expansion after the prompt.
#include <cmath>
#include "common.h"

namespace {

constexpr int kSelThreads = 256;
constexpr int kChunkCols = 2048;      // target columns per partial workgroup: 26 chunks x rows for the 51 865-token vocabulary
constexpr int kMaxChunks = 32;

// Candidate order: NaN first, then larger values, ties to the lower index; an empty slot (index < 0) after everything.
__device__ __forceinline__ bool better(float va, int ia, float vb, int ib) {
  if (ib < 0) return ia >= 0;
  if (ia < 0) return false;
  const bool na = va != va, nb = vb != vb;
  if (na != nb) return na;
  if (!na && va != vb) return va > vb;
  return ia < ib;
}

template <int KP>
__device__ __forceinline__ void insert(float (&tv)[KP], int (&ti)[KP], float v, int i) {
  if (!better(v, i, tv[KP - 1], ti[KP - 1])) return;
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    if (better(v, i, tv[j], ti[j])) {
      const float t = tv[j]; tv[j] = v; v = t;
      const int u = ti[j]; ti[j] = i; i = u;
    }
  }
}

// (max, sum exp(x - max)) pairs; -inf terms contribute nothing, NaN propagates into the sum.
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) { m = mm; s = 0.f; return; }
  const float a = m == -INFINITY ? 0.f : s * expf(m - mm);
  const float b = m2 == -INFINITY ? 0.f : s2 * expf(m2 - mm);
  m = mm; s = a + b;
}

// Merges the 256 threads' sorted lists (registers) into thread 0's registers; fixed pairing, so the result is reproducible.
template <int KP>
__device__ __forceinline__ void block_merge(float (&tv)[KP], int (&ti)[KP], float (*lv)[KP], int (*li)[KP]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < KP; ++j) { lv[t][j] = tv[j]; li[t][j] = ti[j]; }
  __syncthreads();
  for (int half = kSelThreads / 2; half > 0; half >>= 1) {
    if (t < half) {
      int ia = 0, ib = 0;
#pragma unroll
      for (int o = 0; o < KP; ++o) {
        const float va = ia < KP ? lv[t][ia] : 0.f, vb = ib < KP ? lv[t + half][ib] : 0.f;
        const int xa = ia < KP ? li[t][ia] : -1, xb = ib < KP ? li[t + half][ib] : -1;
        if (better(va, xa, vb, xb)) { tv[o] = va; ti[o] = xa; ++ia; } else { tv[o] = vb; ti[o] = xb; ++ib; }
      }
    }
    __syncthreads();
    if (t < half) {
#pragma unroll
      for (int j = 0; j < KP; ++j) { lv[t][j] = tv[j]; li[t][j] = ti[j]; }
    }
    __syncthreads();
  }
}

template <int KP>
__global__ __launch_bounds__(kSelThreads) void select_partial_kernel(const float* __restrict__ logits, int64_t ld, int vocab, int cw,
                                                                     const uint32_t* __restrict__ banned, int log_softmax, float* __restrict__ ws_ms,
                                                                     float* __restrict__ ws_v, int* __restrict__ ws_i) {
  __shared__ float lv[kSelThreads][KP];
  __shared__ int li[kSelThreads][KP];
  __shared__ float wm[kSelThreads / 64], wsum[kSelThreads / 64];
  const int row = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
  const int c0 = ch * cw, c1 = min(vocab, c0 + cw);
  const float* x = logits + (int64_t)row * ld;
  float m = -INFINITY, s = 0.f;
  float tv[KP];
  int ti[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) { tv[j] = 0.f; ti[j] = -1; }
  for (int c = c0 + 4 * threadIdx.x; c < c1; c += 4 * kSelThreads) {
    const float4 q = *reinterpret_cast<const float4*>(x + c);      // c % 4 == 0 and ld % 4 == 0: stays below round_up(vocab, 4) <= ld
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c + j;
      if (col < c1) {
        float v = e[j];
        if (log_softmax && v != -INFINITY) {
          if (v > m) { s = s * expf(m - v) + 1.f; m = v; }
          else s += expf(v - m);
        }
        if (banned && ((banned[col >> 5] >> (col & 31)) & 1u)) v = -INFINITY;
        insert<KP>(tv, ti, v, col);
      }
    }
  }
  if (log_softmax) {
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
      lse_merge(m, s, m2, s2);
    }
    if ((threadIdx.x & 63) == 0) { wm[threadIdx.x >> 6] = m; wsum[threadIdx.x >> 6] = s; }
  }
  block_merge<KP>(tv, ti, lv, li);                                   // its barriers also publish wm / wsum
  if (threadIdx.x == 0) {
    const int64_t rc = (int64_t)row * nch + ch;
    if (log_softmax) {
      m = wm[0]; s = wsum[0];
      for (int w = 1; w < kSelThreads / 64; ++w) lse_merge(m, s, wm[w], wsum[w]);
    }
    ws_ms[2 * rc] = m;
    ws_ms[2 * rc + 1] = s;
#pragma unroll
    for (int j = 0; j < KP; ++j) { ws_v[rc * KP + j] = tv[j]; ws_i[rc * KP + j] = ti[j]; }
  }
}

template <int KP>
__global__ __launch_bounds__(kSelThreads) void select_final_kernel(const float* __restrict__ ws_ms, const float* __restrict__ ws_v, const int* __restrict__ ws_i,
                                                                   int nch, int beams, int vocab, int k, int log_softmax, const float* __restrict__ beam_scores,
                                                                   float* __restrict__ top_scores, int64_t* __restrict__ top_tokens, int32_t* __restrict__ top_parent) {
  __shared__ float lv[kSelThreads][KP];
  __shared__ int li[kSelThreads][KP];
  __shared__ float rmax[8], rlog[8], rbs[8];
  const int clip = blockIdx.x;
  if (threadIdx.x < beams) {
    const int row = clip * beams + threadIdx.x;
    float m = -INFINITY, s = 0.f;
    if (log_softmax)
      for (int ch = 0; ch < nch; ++ch) lse_merge(m, s, ws_ms[2 * ((int64_t)row * nch + ch)], ws_ms[2 * ((int64_t)row * nch + ch) + 1]);
    rmax[threadIdx.x] = m;
    rlog[threadIdx.x] = logf(s);
    rbs[threadIdx.x] = beam_scores ? beam_scores[row] : 0.f;
  }
  __syncthreads();
  float tv[KP];
  int ti[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) { tv[j] = 0.f; ti[j] = -1; }
  const int n = beams * nch * KP;
  for (int c = threadIdx.x; c < n; c += kSelThreads) {
    const int b = c / (nch * KP);
    const int64_t slot = (int64_t)clip * beams * nch * KP + c;
    const int col = ws_i[slot];
    if (col < 0) continue;
    float v = ws_v[slot];
    if (log_softmax) v = v == -INFINITY ? -INFINITY : (v - rmax[b]) - rlog[b];
    if (beam_scores) v = v + rbs[b];
    insert<KP>(tv, ti, v, b * vocab + col);
  }
  block_merge<KP>(tv, ti, lv, li);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < KP; ++j) {
      if (j < k) {
        const int64_t o = (int64_t)clip * k + j;
        top_scores[o] = tv[j];
        top_tokens[o] = ti[j] % vocab;
        if (top_parent) top_parent[o] = ti[j] / vocab;
      }
    }
  }
}

struct SelectPlan { int kp, cw, nch; };

SelectPlan select_plan(int vocab, int k) {
  SelectPlan p;
  p.kp = k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
  int n0 = std::min(kMaxChunks, std::max(1, (vocab + kChunkCols - 1) / kChunkCols));
  p.cw = ((vocab + n0 - 1) / n0 + 3) & ~3;
  p.nch = (vocab + p.cw - 1) / p.cw;
  return p;
}

template <int KP>
void launch_select(const SelectPlan& p, const float* logits, int ld, int rows, int vocab, int beams, const uint32_t* banned, const float* beam_scores,
                   int log_softmax, int k, float* top_scores, int64_t* top_tokens, int32_t* top_parent, float* ms, float* v, int* idx, hipStream_t s) {
  hipLaunchKernelGGL(select_partial_kernel<KP>, dim3(p.nch, rows), dim3(kSelThreads), 0, s, logits, (int64_t)ld, vocab, p.cw, banned, log_softmax, ms, v, idx);
  hipLaunchKernelGGL(select_final_kernel<KP>, dim3(rows / beams), dim3(kSelThreads), 0, s, ms, v, idx, p.nch, beams, vocab, k, log_softmax, beam_scores,
                     top_scores, top_tokens, top_parent);
}

__global__ __launch_bounds__(256) void kv_gather_kernel(const float4* __restrict__ src, float4* __restrict__ dst, const int32_t* __restrict__ parent,
                                                        int src_rows, int dst_rows, int T, int Tmax, int w4, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % w4);
    int64_t q = i / w4;
    const int t = (int)(q % T); q /= T;
    const int r = (int)(q % dst_rows);
    const int64_t l = q / dst_rows;
    const int p = parent[r];
    if (p < 0 || p >= src_rows) continue;                           // out-of-range parent: the destination row is left as it was
    dst[((l * dst_rows + r) * Tmax + t) * w4 + c] = src[((l * src_rows + p) * Tmax + t) * w4 + c];
  }
}

}  // namespace

extern "C" size_t awt_select_tokens_workspace_bytes(int rows, int vocab, int k) {
  if (rows <= 0 || vocab <= 0 || k <= 0 || k > 16) return 0;
  const SelectPlan p = select_plan(vocab, k);
  return (size_t)rows * p.nch * (2 + 2 * p.kp) * 4 + 256;
}

extern "C" int awt_op_select_tokens(awt_ctx* c, const float* logits, int ld, int rows, int vocab, int beams, const uint32_t* banned,
                                    const float* beam_scores, int log_softmax, int k, float* top_scores, int64_t* top_tokens, int32_t* top_parent,
                                    void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && logits && top_scores && top_tokens && workspace, AWT_ERR_INVALID, "op_select_tokens: null argument");
  AWT_REQUIRE(beams >= 1 && beams <= 8, AWT_ERR_INVALID, "op_select_tokens: beams must be in [1, 8]");
  AWT_REQUIRE(k >= 1 && k <= 16, AWT_ERR_INVALID, "op_select_tokens: k must be in [1, 16]");
  AWT_REQUIRE(rows >= 1 && rows % beams == 0, AWT_ERR_INVALID, "op_select_tokens: rows must be a positive multiple of beams");
  AWT_REQUIRE(vocab >= 1 && ld >= vocab && ld % 4 == 0, AWT_ERR_INVALID, "op_select_tokens: need 1 <= vocab <= ld and ld % 4 == 0");
  AWT_REQUIRE((int64_t)k <= (int64_t)beams * vocab, AWT_ERR_INVALID, "op_select_tokens: k exceeds the beams x vocab candidates");
  AWT_REQUIRE((int64_t)beams * vocab < (1ll << 31), AWT_ERR_INVALID, "op_select_tokens: beams x vocab must fit in 31 bits");
  AWT_REQUIRE(((uintptr_t)logits & 15) == 0, AWT_ERR_INVALID, "op_select_tokens: logits must be 16-byte aligned (float4 loads)");
  const SelectPlan p = select_plan(vocab, k);
  const size_t need = awt_select_tokens_workspace_bytes(rows, vocab, k);
  AWT_REQUIRE(ws_bytes >= need, AWT_ERR_INVALID, "op_select_tokens: workspace too small (" + std::to_string(ws_bytes) + " < " + std::to_string(need) + " bytes)");
  const int64_t rc = (int64_t)rows * p.nch;
  float* ms = static_cast<float*>(workspace);
  float* v = ms + 2 * rc;
  int* idx = reinterpret_cast<int*>(v + rc * p.kp);
  hipStream_t s = (hipStream_t)stream;
  switch (p.kp) {
    case 1: launch_select<1>(p, logits, ld, rows, vocab, beams, banned, beam_scores, log_softmax, k, top_scores, top_tokens, top_parent, ms, v, idx, s); break;
    case 2: launch_select<2>(p, logits, ld, rows, vocab, beams, banned, beam_scores, log_softmax, k, top_scores, top_tokens, top_parent, ms, v, idx, s); break;
    case 4: launch_select<4>(p, logits, ld, rows, vocab, beams, banned, beam_scores, log_softmax, k, top_scores, top_tokens, top_parent, ms, v, idx, s); break;
    case 8: launch_select<8>(p, logits, ld, rows, vocab, beams, banned, beam_scores, log_softmax, k, top_scores, top_tokens, top_parent, ms, v, idx, s); break;
    default: launch_select<16>(p, logits, ld, rows, vocab, beams, banned, beam_scores, log_softmax, k, top_scores, top_tokens, top_parent, ms, v, idx, s); break;
  }
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" int awt_op_kv_gather(awt_ctx* c, const float* src, float* dst, const int32_t* parent, int layers, int src_rows, int dst_rows, int T, int Tmax,
                                int width, void* stream) {
  AWT_REQUIRE(c && src && dst && parent, AWT_ERR_INVALID, "op_kv_gather: null argument");
  AWT_REQUIRE(src != dst, AWT_ERR_INVALID, "op_kv_gather: source and destination must be different buffers");
  AWT_REQUIRE(layers >= 1 && src_rows >= 1 && dst_rows >= 1 && T >= 1 && T <= Tmax, AWT_ERR_INVALID,
              "op_kv_gather: need layers, rows >= 1 and 1 <= T <= Tmax");
  AWT_REQUIRE(width >= 4 && width % 4 == 0, AWT_ERR_INVALID, "op_kv_gather: width must be a positive multiple of 4");
  AWT_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, AWT_ERR_INVALID, "op_kv_gather: buffers must be 16-byte aligned");
  const int w4 = width / 4;
  const int64_t total = (int64_t)layers * dst_rows * T * w4;
  const int grid = (int)std::min<int64_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(kv_gather_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(src), reinterpret_cast<float4*>(dst),
                     parent, src_rows, dst_rows, T, Tmax, w4, total);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}
