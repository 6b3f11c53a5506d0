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
// awt_op_select_tokens_ts adds HF's WhisperTimeStampLogitsProcessor (transformers/generation/logits_process.py) to the same two launches.
// Each partial workgroup derives its row's state from the row's own token history after the prompt (last two tokens, last timestamp)
// and bans <|notimestamps|>, the pair rule's and the monotonic rule's columns and, at the first generated step, the text columns and
// the timestamps beyond max_initial_timestamp_index.  The chunk grid is split at timestamp_begin, so that a chunk holds only text or
// only timestamp columns, and each chunk also emits (max, sum exp) of its banned row (NaN flagged).  The final workgroup decides per row
// whether logsumexp(timestamps) > max(text) (the forcing rule; a NaN does not force) and, when it does, turns that row's text
// candidates into -inf.  The log-softmax stays the one over the unbanned row, as HF's beam search feeds log_softmax(logits) to the
// processors; the forcing comparison is shift-invariant, so raw logits and log-probabilities decide it alike.
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

// Timestamp rules of one selection (awt_ts_rules plus the chunk split at timestamp_begin: n_t text chunks of cw_t columns, then
// timestamp chunks of cw_s columns).
struct TsParams {
  const int64_t* hist; int64_t hist_ld;
  int begin, cur_len, eos, no_ts, tb, mii;
  int n_t, cw_t, cw_s;
};

// The row's rule state from history[begin, cur_len): whether the last / second-last token is a timestamp and the first banned-below
// limit of the monotonic rule (tb when there is no timestamp yet).  Every thread gets the result; uses two barriers.
__device__ __forceinline__ void ts_row_state(const TsParams& t, int row, int* red, bool& last_ts, bool& pen_ts, int& ts_lim) {
  const int64_t* h = t.hist + (int64_t)row * t.hist_ld;
  const int n = t.cur_len - t.begin;
  int pos = -1;
  for (int i = threadIdx.x; i < n; i += kSelThreads)
    if (h[t.begin + i] >= t.tb) pos = i;                              // i grows per thread: the thread's last hit
  for (int o = 32; o > 0; o >>= 1) pos = max(pos, __shfl_xor(pos, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = pos;
  __syncthreads();
  pos = red[0];
  for (int w = 1; w < kSelThreads / 64; ++w) pos = max(pos, red[w]);
  __syncthreads();
  last_ts = n >= 1 && h[t.cur_len - 1] >= t.tb;
  pen_ts = n < 2 || h[t.cur_len - 2] >= t.tb;
  ts_lim = t.tb;
  if (pos >= 0) {
    const int last = (int)h[t.begin + pos];
    ts_lim = (last_ts && !pen_ts) ? last : last + 1;
  }
}

template <int KP, bool TS>
__global__ __launch_bounds__(kSelThreads) void select_partial_kernel(const float* __restrict__ logits, int64_t ld, int vocab, int cw,
                                                                     const uint32_t* __restrict__ banned, int log_softmax, float* __restrict__ ws_ms,
                                                                     float* __restrict__ ws_v, int* __restrict__ ws_i, TsParams tp,
                                                                     float* __restrict__ ws_mm) {
  __shared__ float lv[kSelThreads][KP];
  __shared__ int li[kSelThreads][KP];
  __shared__ float wm[kSelThreads / 64], wsum[kSelThreads / 64];
  __shared__ float wmm[TS ? kSelThreads / 64 : 1], wsm[TS ? kSelThreads / 64 : 1];
  __shared__ int wnan[TS ? kSelThreads / 64 : 1];
  const int row = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
  int c0 = ch * cw, c1 = min(vocab, c0 + cw);
  bool last_ts = false, pen_ts = false, first = false;
  int ts_lim = 0;
  if constexpr (TS) {
    if (ch < tp.n_t) { c0 = ch * tp.cw_t; c1 = min(tp.tb, c0 + tp.cw_t); }
    else { c0 = tp.tb + (ch - tp.n_t) * tp.cw_s; c1 = min(vocab, c0 + tp.cw_s); }
    ts_row_state(tp, row, reinterpret_cast<int*>(wnan), last_ts, pen_ts, ts_lim);
    first = tp.cur_len == tp.begin;
  }
  const float* x = logits + (int64_t)row * ld;
  float m = -INFINITY, s = 0.f;
  float mm = -INFINITY, sm = 0.f;                                     // (max, sum exp) of the banned row (rules only)
  int nan = 0;
  float tv[KP];
  int ti[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) { tv[j] = 0.f; ti[j] = -1; }
  // rules: chunk starts need not be 4-aligned (timestamp_begin 50365); the float4 walk starts at the aligned column below c0
  for (int c = (TS ? (c0 & ~3) : c0) + 4 * threadIdx.x; c < c1; c += 4 * kSelThreads) {
    const float4 q = *reinterpret_cast<const float4*>(x + c);      // c % 4 == 0 and ld % 4 == 0: stays below round_up(vocab, 4) <= ld
    const float e[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c + j;
      if (col < c1 && (!TS || col >= c0)) {
        float v = e[j];
        if (log_softmax && v != -INFINITY) {
          if (v > m) { s = s * expf(m - v) + 1.f; m = v; }
          else s += expf(v - m);
        }
        if (banned && ((banned[col >> 5] >> (col & 31)) & 1u)) v = -INFINITY;
        if constexpr (TS) {
          const bool ts = col >= tp.tb;
          if (col == tp.no_ts || (last_ts && pen_ts && ts) || (last_ts && !pen_ts && col < tp.eos) || (ts && col < ts_lim) ||
              (first && !ts) || (first && tp.mii >= 0 && col > tp.tb + tp.mii))
            v = -INFINITY;
          if (v != v) nan = 1;
          else if (v != -INFINITY) {
            if (v > mm) { sm = sm * expf(mm - v) + 1.f; mm = v; }
            else sm += expf(v - mm);
          }
        }
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
  if constexpr (TS) {
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(mm, o), s2 = __shfl_xor(sm, o);
      lse_merge(mm, sm, m2, s2);
      nan |= __shfl_xor(nan, o);
    }
    if ((threadIdx.x & 63) == 0) { wmm[threadIdx.x >> 6] = mm; wsm[threadIdx.x >> 6] = sm; wnan[threadIdx.x >> 6] = nan; }
  }
  block_merge<KP>(tv, ti, lv, li);                                   // its barriers also publish wm / wsum (and wmm / wsm / wnan)
  if (threadIdx.x == 0) {
    const int64_t rc = (int64_t)row * nch + ch;
    if (log_softmax) {
      m = wm[0]; s = wsum[0];
      for (int w = 1; w < kSelThreads / 64; ++w) lse_merge(m, s, wm[w], wsum[w]);
    }
    ws_ms[2 * rc] = m;
    ws_ms[2 * rc + 1] = s;
    if constexpr (TS) {
      mm = wmm[0]; sm = wsm[0]; nan = wnan[0];
      for (int w = 1; w < kSelThreads / 64; ++w) { lse_merge(mm, sm, wmm[w], wsm[w]); nan |= wnan[w]; }
      ws_mm[2 * rc] = nan ? NAN : mm;
      ws_mm[2 * rc + 1] = sm;
    }
#pragma unroll
    for (int j = 0; j < KP; ++j) { ws_v[rc * KP + j] = tv[j]; ws_i[rc * KP + j] = ti[j]; }
  }
}

template <int KP, bool TS>
__global__ __launch_bounds__(kSelThreads) void select_final_kernel(const float* __restrict__ ws_ms, const float* __restrict__ ws_v, const int* __restrict__ ws_i,
                                                                   int nch, int beams, int vocab, int k, int log_softmax, const float* __restrict__ beam_scores,
                                                                   float* __restrict__ top_scores, int64_t* __restrict__ top_tokens, int32_t* __restrict__ top_parent,
                                                                   const float* __restrict__ ws_mm, int n_t) {
  __shared__ float lv[kSelThreads][KP];
  __shared__ int li[kSelThreads][KP];
  __shared__ float rmax[8], rlog[8], rbs[8];
  __shared__ int rforce[8];
  const int clip = blockIdx.x;
  if (threadIdx.x < beams) {
    const int row = clip * beams + threadIdx.x;
    float m = -INFINITY, s = 0.f;
    if (log_softmax)
      for (int ch = 0; ch < nch; ++ch) lse_merge(m, s, ws_ms[2 * ((int64_t)row * nch + ch)], ws_ms[2 * ((int64_t)row * nch + ch) + 1]);
    rmax[threadIdx.x] = m;
    rlog[threadIdx.x] = logf(s);
    rbs[threadIdx.x] = beam_scores ? beam_scores[row] : 0.f;
    if constexpr (TS) {
      // forcing rule: logsumexp(timestamps) > max(text) of the banned row, chunk order; a NaN anywhere makes the comparison false
      bool nan = false;
      float mt = -INFINITY, ms = -INFINITY, ss = 0.f;
      for (int ch = 0; ch < nch; ++ch) {
        const float a = ws_mm[2 * ((int64_t)row * nch + ch)], b = ws_mm[2 * ((int64_t)row * nch + ch) + 1];
        if (a != a) nan = true;
        else if (ch < n_t) mt = fmaxf(mt, a);
        else lse_merge(ms, ss, a, b);
      }
      rforce[threadIdx.x] = !nan && (ms + logf(ss)) > mt;
    }
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
    if constexpr (TS) {
      if (rforce[b] && (c / KP) % nch < n_t) v = -INFINITY;           // forced row: its text columns are banned
    }
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

// With timestamp rules: text columns [0, tb) and timestamp columns [tb, vocab) chunked separately (26 chunks for 51 865 / 51 866).
void ts_plan(int vocab, int tb, SelectPlan& p, TsParams& t) {
  t.n_t = std::max(1, (tb + kChunkCols - 1) / kChunkCols);
  t.cw_t = (tb + t.n_t - 1) / t.n_t;
  const int nts = vocab - tb;
  const int n_s = std::max(1, (nts + kChunkCols - 1) / kChunkCols);
  t.cw_s = (nts + n_s - 1) / n_s;
  p.nch = t.n_t + n_s;
  p.cw = 0;
}

template <int KP, bool TS>
void launch_select(const SelectPlan& p, const float* logits, int ld, int rows, int vocab, int beams, const uint32_t* banned, const float* beam_scores,
                   int log_softmax, int k, float* top_scores, int64_t* top_tokens, int32_t* top_parent, float* ms, float* v, int* idx, const TsParams& tp,
                   float* mm, hipStream_t s) {
  hipLaunchKernelGGL((select_partial_kernel<KP, TS>), dim3(p.nch, rows), dim3(kSelThreads), 0, s, logits, (int64_t)ld, vocab, p.cw, banned, log_softmax, ms,
                     v, idx, tp, mm);
  hipLaunchKernelGGL((select_final_kernel<KP, TS>), dim3(rows / beams), dim3(kSelThreads), 0, s, ms, v, idx, p.nch, beams, vocab, k, log_softmax, beam_scores,
                     top_scores, top_tokens, top_parent, mm, tp.n_t);
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

extern "C" size_t awt_select_tokens_ts_workspace_bytes(int rows, int vocab, int k) {
  if (rows <= 0 || vocab <= 0 || k <= 0 || k > 16) return 0;
  const SelectPlan p = select_plan(vocab, k);
  return (size_t)rows * (kMaxChunks + 2) * (4 + 2 * p.kp) * 4 + 256;      // either chunk grid, plus the banned-row pairs
}

extern "C" int awt_op_select_tokens_ts(awt_ctx* c, const float* logits, int ld, int rows, int vocab, int beams, const uint32_t* banned,
                                       const float* beam_scores, int log_softmax, int k, const awt_ts_rules* rules, float* top_scores,
                                       int64_t* top_tokens, int32_t* top_parent, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && logits && top_scores && top_tokens && workspace, AWT_ERR_INVALID, "op_select_tokens: null argument");
  AWT_REQUIRE(beams >= 1 && beams <= 8, AWT_ERR_INVALID, "op_select_tokens: beams must be in [1, 8]");
  AWT_REQUIRE(k >= 1 && k <= 16, AWT_ERR_INVALID, "op_select_tokens: k must be in [1, 16]");
  AWT_REQUIRE(rows >= 1 && rows % beams == 0, AWT_ERR_INVALID, "op_select_tokens: rows must be a positive multiple of beams");
  AWT_REQUIRE(vocab >= 1 && ld >= vocab && ld % 4 == 0, AWT_ERR_INVALID, "op_select_tokens: need 1 <= vocab <= ld and ld % 4 == 0");
  AWT_REQUIRE((int64_t)k <= (int64_t)beams * vocab, AWT_ERR_INVALID, "op_select_tokens: k exceeds the beams x vocab candidates");
  AWT_REQUIRE((int64_t)beams * vocab < (1ll << 31), AWT_ERR_INVALID, "op_select_tokens: beams x vocab must fit in 31 bits");
  AWT_REQUIRE(((uintptr_t)logits & 15) == 0, AWT_ERR_INVALID, "op_select_tokens: logits must be 16-byte aligned (float4 loads)");
  SelectPlan p = select_plan(vocab, k);
  const size_t need = rules ? awt_select_tokens_ts_workspace_bytes(rows, vocab, k) : awt_select_tokens_workspace_bytes(rows, vocab, k);
  AWT_REQUIRE(ws_bytes >= need, AWT_ERR_INVALID, "op_select_tokens: workspace too small (" + std::to_string(ws_bytes) + " < " + std::to_string(need) + " bytes)");
  TsParams tp{};
  if (rules) {
    const int tb = rules->no_timestamps_token_id + 1;
    AWT_REQUIRE(rules->history, AWT_ERR_INVALID, "op_select_tokens_ts: null token history");
    AWT_REQUIRE(rules->no_timestamps_token_id >= 1 && tb < vocab, AWT_ERR_INVALID,
                "op_select_tokens_ts: need timestamp tokens: 1 <= no_timestamps_token_id < vocab - 1");
    AWT_REQUIRE(rules->eos_token_id >= 0 && rules->eos_token_id < tb, AWT_ERR_INVALID, "op_select_tokens_ts: need 0 <= eos_token_id < timestamp_begin");
    AWT_REQUIRE(rules->begin >= 0 && rules->cur_len >= rules->begin && rules->hist_ld >= rules->cur_len, AWT_ERR_INVALID,
                "op_select_tokens_ts: need 0 <= begin <= cur_len <= hist_ld");
    tp.hist = rules->history; tp.hist_ld = rules->hist_ld; tp.begin = rules->begin; tp.cur_len = rules->cur_len;
    tp.eos = rules->eos_token_id; tp.no_ts = rules->no_timestamps_token_id; tp.tb = tb;
    tp.mii = rules->max_initial_timestamp_index;
    ts_plan(vocab, tb, p, tp);
    AWT_REQUIRE(p.nch <= kMaxChunks + 2, AWT_ERR_INVALID, "op_select_tokens_ts: vocabulary too large for the chunk grid");
  }
  const int64_t rc = (int64_t)rows * p.nch;
  float* ms = static_cast<float*>(workspace);
  float* v = ms + 2 * rc;
  int* idx = reinterpret_cast<int*>(v + rc * p.kp);
  float* mm = reinterpret_cast<float*>(idx + rc * p.kp);
  hipStream_t s = (hipStream_t)stream;
#define AWT_SELECT_CASE(KP)                                                                                                              \
  if (rules) launch_select<KP, true>(p, logits, ld, rows, vocab, beams, banned, beam_scores, log_softmax, k, top_scores, top_tokens, top_parent, ms, v, \
                                     idx, tp, mm, s);                                                                                     \
  else launch_select<KP, false>(p, logits, ld, rows, vocab, beams, banned, beam_scores, log_softmax, k, top_scores, top_tokens, top_parent, ms, v, idx, \
                                tp, nullptr, s);
  switch (p.kp) {
    case 1: AWT_SELECT_CASE(1) break;
    case 2: AWT_SELECT_CASE(2) break;
    case 4: AWT_SELECT_CASE(4) break;
    case 8: AWT_SELECT_CASE(8) break;
    default: AWT_SELECT_CASE(16) break;
  }
#undef AWT_SELECT_CASE
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}

extern "C" int awt_op_select_tokens(awt_ctx* c, const float* logits, int ld, int rows, int vocab, int beams, const uint32_t* banned,
                                    const float* beam_scores, int log_softmax, int k, float* top_scores, int64_t* top_tokens, int32_t* top_parent,
                                    void* workspace, size_t ws_bytes, void* stream) {
  return awt_op_select_tokens_ts(c, logits, ld, rows, vocab, beams, banned, beam_scores, log_softmax, k, nullptr, top_scores, top_tokens, top_parent,
                                 workspace, ws_bytes, stream);
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
