// Multi-head cross-attention for head_dim 128, no mask, Lq != Sk, on fp32 row-major operands in place -- gfx950.
//
//   o[b, i, h] = softmax_j(128^-1/2 q[b, i, h] . k[b, j, h]) v[b, j, h]        row (b, i) of q at q + (b Lq + i) ldq + 128 h,
//                                                                               row (b, j) of k / v at k + (b Sk + j) ldk + 128 h, o like q with ldo
// The consumer is music2midi.CrossAttentionAdapter: 8 heads over a hidden size of 1024, 512 text positions against 1500 encoder positions, k and v the two
// halves of ONE [B Sk, 2 H 128] GEMM output.  Nothing is pre-split into planes: every kernel splits fp32 into bf16 hi (+ lo) on the way into LDS or into its
// lane-resident fragments, so the operator reads and writes fp32 tensors only (DESIGN.md section 4.11 has the byte counts).
//
// All three kernels have the shape of attention.hip / attention_bwd.hip: four waves, 32 lane-resident rows per wave (queries; in the dk / dv launch keys),
// tiles of the other operand streamed through LDS.  The first products are "tile rows x lane-resident fragments" on v_mfma_f32_32x32x16_bf16; their 32 x 32
// accumulators (reduction index in the registers, lane-resident index on the lane) are converted to bf16 in place and are the B operands of the second
// products, whose A operands are TRANSPOSED tile images [128 dims][tile rows].  Those are a second LDS image written by the staging pass (the split has to
// pass through registers anyway, so no ds_read_tr is needed) with the tile rows of each 16-block stored in the k order of an accumulator used as an operand:
// position 8 h + 4 a + b holds row 8 a + 4 h + b.
//   forward   S^T = K Q^T (64 keys x 32 queries per wave and tile), online softmax per lane (fp32 running max, sum, 128-dim output), O^T += V^T P^T
//   dq        S^T and dP^T = V dO^T, P = exp2(s - lse2), dS^T = P (dP - delta), dQ^T += K^T dS^T
//   dk / dv   S = Q K^T and dP = dO V^T (32 queries x 32 keys per wave and tile), dV^T += dO^T P, dK^T += Q^T dS; 64 keys per workgroup, the two waves of a
//             key block each form 64 of the 128 dims (k, v fragments and both 128-dim accumulators do not fit one wave's registers; S and dP are formed twice)
// delta = rowsum(dO * O) comes from a small launch of its own into the workspace.  No atomics anywhere: two runs give the same bits.
// CAUSAL variants of all three (awt_op_causal_attention, _lse, _backward: a decode cache with grouped KV heads, Qwen3Decoder) are compile-time branches.
// TERMS = 3: every operand is a hi + lo bf16 pair, three MFMAs per fragment pair (a_lo b_hi + a_hi b_lo + a_hi b_hi); TERMS = 1: hi only.
#include <algorithm>
#include "common.h"

namespace {

constexpr int XD = 128;            // head_dim
constexpr int XTHREADS = 256;
constexpr int XLW = 32;            // lane-resident rows per wave
constexpr int XLB = 128;           // ... per workgroup
constexpr int XKT = 64;            // keys per streamed tile (forward, dq)
constexpr int XQT = 32;            // queries per streamed tile (dk / dv)
constexpr int XKB = 64;            // keys per workgroup of the dk / dv launch: two waves share 32 keys, each forms 64 of the 128 dims of dk and dv
constexpr int XRP = XD + 8;        // pitch of a row image [rows][128] in 16-bit elements: 272 bytes, so that the 16 rows of a ds_read_b128 group start 4 banks apart
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

struct XArgs {
  const float *q, *k, *v;
  const float* o; const float* dout; const float* lse_in; const float* delta_in;    // backward inputs (o, dout pitched like the forward's o)
  float* out; float* lse; float* delta; float *dq, *dk, *dv;
  int B, H, Lq, Sk;
  int64_t ldq, ldk, ldv, ldo;
  float scale;                     // 128^-1/2
  int Hkv; int64_t kvbs;           // causal kernels only: KV heads (query head h reads KV head h / (H / Hkv)) and the cache's batch stride; Sk is then T
  int64_t lddkv, dkvbs;            // causal dk / dv launch only: row pitch and batch stride of dk / dv (the cache's layout, Hkv heads)
};

template <bool LO>
__device__ __forceinline__ f32x16 mma3(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x16 c) {
  if constexpr (LO) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
  }
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 lds_frag(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

// the lane's operand fragments of one fp32 row of 128: k-step s holds elements 16 s + 8 h + 0..7 (both the A and the B map of the 32 x 32 x 16 MFMA)
template <bool LO>
__device__ __forceinline__ void load_frags(const float* row, int h, bf16x8 (&fh)[8], bf16x8 (&fl)[8]) {
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const float4 x0 = *reinterpret_cast<const float4*>(row + 16 * s + 8 * h), x1 = *reinterpret_cast<const float4*>(row + 16 * s + 8 * h + 4);
    const float x[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bf16_t a, b;
      split_bf16(x[j], a, b);
      fh[s][j] = (short)a;
      fl[s][j] = (short)b;
    }
    if constexpr (!LO) fl[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}

// ---- staging of a tile of ROWS rows x 128 dims, fp32 in global memory.  `base` points at dim 0 of the tile's first row; rows >= valid (valid >= 1) become
// zero.  The loads are unconditional, from the row clamped to the last valid one, and the WRITE pass selects the zero: with `row < valid ? load : 0` hipcc
// branches around each load and (in the one-product instantiations) waits for each before the next -- a tile's loads become that many serial round trips --
// and a select right after the load makes the forward wait for its prefetch before the products it should fly under.
// Row image [ROWS][XRP]: thread t takes the float4 pieces t, t + 256, ... of the tile (32 pieces per row).
template <int ROWS>
__device__ __forceinline__ void load_rows(const float* base, int64_t ld, int valid, int tid, float4 (&r)[ROWS / 8]) {
#pragma unroll
  for (int i = 0; i < ROWS / 8; ++i) {
    const int idx = i * XTHREADS + tid, row = idx >> 5, c4 = idx & 31;
    r[i] = *reinterpret_cast<const float4*>(base + (int64_t)min(row, valid - 1) * ld + 4 * c4);
  }
}
template <int ROWS, bool LO>
__device__ __forceinline__ void write_rows(const float4 (&r)[ROWS / 8], int valid, int tid, bf16_t* hi, bf16_t* lo) {
#pragma unroll
  for (int i = 0; i < ROWS / 8; ++i) {
    const int idx = i * XTHREADS + tid, row = idx >> 5, c4 = idx & 31;
    const float x[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
    bf16_t a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) split_bf16(row < valid ? x[t] : 0.f, a[t], b[t]);
    *reinterpret_cast<uint2*>(hi + row * XRP + 4 * c4) = make_uint2(pack2(a[0], a[1]), pack2(a[2], a[3]));
    if constexpr (LO) *reinterpret_cast<uint2*>(lo + row * XRP + 4 * c4) = make_uint2(pack2(b[0], b[1]), pack2(b[2], b[3]));
  }
}
// Transposed image [128][ROWS + 8]: thread t owns dim t & 127 and the groups g = (t >> 7) + 2 i of four consecutive rows; the four values of a group are
// one 8-byte store at position 16 (g >> 2) + 8 (g & 1) + 4 ((g >> 1) & 1) -- rows 8 a + 4 h + b of a 16-block at positions 8 h + 4 a + b.
template <int ROWS>
__device__ __forceinline__ void load_cols(const float* base, int64_t ld, int valid, int tid, float (&r)[ROWS / 2]) {
  const int d = tid & 127, g0 = tid >> 7;
#pragma unroll
  for (int i = 0; i < ROWS / 8; ++i)
#pragma unroll
    for (int b = 0; b < 4; ++b) r[4 * i + b] = base[(int64_t)min(4 * (g0 + 2 * i) + b, valid - 1) * ld + d];
}
template <int ROWS, bool LO>
__device__ __forceinline__ void write_cols(const float (&r)[ROWS / 2], int valid, int tid, bf16_t* hi, bf16_t* lo) {
  const int d = tid & 127, g0 = tid >> 7;
#pragma unroll
  for (int i = 0; i < ROWS / 8; ++i) {
    const int g = g0 + 2 * i, pos = 16 * (g >> 2) + 8 * (g & 1) + 4 * ((g >> 1) & 1);
    bf16_t a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) split_bf16(4 * g + t < valid ? r[4 * i + t] : 0.f, a[t], b[t]);
    *reinterpret_cast<uint2*>(hi + d * (ROWS + 8) + pos) = make_uint2(pack2(a[0], a[1]), pack2(a[2], a[3]));
    if constexpr (LO) *reinterpret_cast<uint2*>(lo + d * (ROWS + 8) + pos) = make_uint2(pack2(b[0], b[1]), pack2(b[2], b[3]));
  }
}

// registers 8 s .. 8 s + 7 of a 32 x 32 accumulator as the B fragment of k-step s of the next product
template <bool LO>
__device__ __forceinline__ void acc_frags(const f32x16& x, bf16x8 (&fh)[2], bf16x8 (&fl)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bf16_t a, b;
      split_bf16(x[8 * s + j], a, b);
      fh[s][j] = (short)a;
      fl[s][j] = (short)b;
    }
    if constexpr (!LO) fl[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}
// row of accumulator register i in lane half h (MFMA C / D map)
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

// N transposed 32 x 32 accumulators acc[dt] (dim 32 dt + acc_row(i, h) of the dims at `row`, lane-resident row r) times `mul`, as four float4 per 32-dim block
template <int N>
__device__ __forceinline__ void store_acc_t(const f32x16 (&acc)[N], float mul, float* row, int h) {
#pragma unroll
  for (int dt = 0; dt < N; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(row + 32 * dt + 8 * g + 4 * h) =
          make_float4(acc[dt][4 * g] * mul, acc[dt][4 * g + 1] * mul, acc[dt][4 * g + 2] * mul, acc[dt][4 * g + 3] * mul);
}

// LDS bytes: row images of 64 rows, transposed images of 64 (forward, dq) or 32 (dk / dv) rows, one plane
constexpr int XROW64 = XKT * XRP * 2, XCOL64 = XD * (XKT + 8) * 2, XROW32 = XQT * XRP * 2, XCOL32 = XD * (XQT + 8) * 2;
constexpr int fwd_lds(int terms) { return (terms == 3 ? 2 : 1) * (XROW64 + XCOL64); }
constexpr int dq_lds(int terms) { return (terms == 3 ? 2 : 1) * (2 * XROW64 + XCOL64); }
constexpr int dkv_lds(int terms) { return (terms == 3 ? 2 : 1) * (2 * XROW32 + 2 * XCOL32) + 2 * XQT * 4; }

// ------------------------------------------------------------------------------------------------ forward
// CAUSAL (awt_op_causal_attention): k / v are a decode cache -- batch b at k + b kvbs, row pitch ldk = ldv, Hkv heads -- holding a.Sk = T live positions, and query
// i sees keys j <= T - Lq + i.  A workgroup streams key tiles up to its LAST query's diagonal only (`Sk` below: the staging's `valid` bound, so no row past it --
// in particular nothing at a cache position >= T, which is uninitialised memory in real use -- is ever loaded; the rest of the last tile is zeros in LDS), a wave
// skips the tiles past its own last query, and the mask is applied to the scores of the tiles that remain.  Key 0 is visible to every query and tile 0 is
// processed by every live wave, so a row's running maximum is a real score before any fully masked tile reaches it and masked scores weigh exp2(-1e30 - m) = 0.
// The non-causal instantiations compile to what they were: every difference is under `if constexpr` or folds to the old expression.
template <int TERMS, bool CAUSAL = false>
__global__ __launch_bounds__(XTHREADS) void xattn_fwd_kernel(XArgs a) {
  constexpr bool LO = TERMS == 3;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* kh = reinterpret_cast<bf16_t*>(smem);
  bf16_t* kl = kh + (LO ? XKT * XRP : 0);
  bf16_t* vth = kl + XKT * XRP;
  bf16_t* vtl = vth + (LO ? XD * (XKT + 8) : 0);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int nqb = (a.Lq + XLB - 1) / XLB;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb, b = bh / a.H, head = bh - b * a.H;
  const int q0 = qb * XLB + wave * XLW, qi = q0 + r;
  const bool live = q0 < a.Lq;                                     // wave-uniform: a wave past the last query only stages
  const int qc = min(qi, a.Lq - 1);                                // tail queries read the last row and are not stored
  const float *kbase, *vbase;
  int Sk, lim = 0, wlim = 0;                                       // keys this workgroup streams; last visible key of this lane's query / of the wave's last query
  if constexpr (CAUSAL) {
    const int kvh = head / (a.H / a.Hkv), off = a.Sk - a.Lq;
    kbase = a.k + (int64_t)b * a.kvbs + XD * kvh;
    vbase = a.v + (int64_t)b * a.kvbs + XD * kvh;
    Sk = off + min(qb * XLB + XLB, a.Lq);
    lim = off + qc;
    wlim = off + min(q0 + XLW, a.Lq) - 1;
  } else {
    kbase = a.k + (int64_t)b * a.Sk * a.ldk + XD * head;
    vbase = a.v + (int64_t)b * a.Sk * a.ldv + XD * head;
    Sk = a.Sk;
  }

  bf16x8 qh[8], ql[8];
  load_frags<LO>(a.q + ((int64_t)b * a.Lq + qc) * a.ldq + XD * head, h, qh, ql);

  f32x16 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
  float m = -1.0e30f, l = 0.f;
  const float sc2 = a.scale * kLog2e;

  float4 kr[XKT / 8]; float vr[XKT / 2];
  load_rows<XKT>(kbase, a.ldk, Sk, tid, kr);
  load_cols<XKT>(vbase, a.ldv, Sk, tid, vr);
  const int nt = (Sk + XKT - 1) / XKT;
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * XKT;
    __syncthreads();                                               // the previous tile's fragment reads are done
    write_rows<XKT, LO>(kr, Sk - k0, tid, kh, kl);
    write_cols<XKT, LO>(vr, Sk - k0, tid, vth, vtl);
    __syncthreads();
    if (t + 1 < nt) {                                              // the next tile's loads fly under this tile's products
      load_rows<XKT>(kbase + (int64_t)(k0 + XKT) * a.ldk, a.ldk, Sk - k0 - XKT, tid, kr);
      load_cols<XKT>(vbase + (int64_t)(k0 + XKT) * a.ldv, a.ldv, Sk - k0 - XKT, tid, vr);
    }
    if (!live) continue;
    if constexpr (CAUSAL) { if (k0 > wlim) continue; }           // wave-uniform: every key of the tile lies past this wave's last query

    f32x16 st[2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
#pragma unroll
      for (int i = 0; i < 16; ++i) st[blk][i] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int off = (32 * blk + r) * XRP + 16 * s + 8 * h;
        st[blk] = mma3<LO>(lds_frag(kh + off), lds_frag(kl + off), qh[s], ql[s], st[blk]);
      }
    }
    float tmax = -1.0e30f;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kj = k0 + 32 * blk + acc_row(i, h);
        const float x = (CAUSAL ? kj <= lim : kj < Sk) ? st[blk][i] * sc2 : -1.0e30f;   // tail (masked) keys never win and weigh exp2(-1e30 - m) = 0
        st[blk][i] = x;
        tmax = fmaxf(tmax, x);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float m_new = fmaxf(m, tmax), alpha = __builtin_amdgcn_exp2f(m - m_new);
    float psum = 0.f;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = __builtin_amdgcn_exp2f(st[blk][i] - m_new);
        st[blk][i] = p;
        psum += p;
      }
    psum += __shfl_xor(psum, 32);
    l = l * alpha + psum;
    m = m_new;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[dt][i] *= alpha;
    bf16x8 ph[2][2], pl[2][2];
    acc_frags<LO>(st[0], ph[0], pl[0]);
    acc_frags<LO>(st[1], ph[1], pl[1]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int off = (32 * dt + r) * (XKT + 8) + 32 * blk + 16 * s + 8 * h;
          acc[dt] = mma3<LO>(lds_frag(vth + off), lds_frag(vtl + off), ph[blk][s], pl[blk][s], acc[dt]);
        }
  }
  if (live && qi < a.Lq) {
    store_acc_t(acc, 1.0f / l, a.out + ((int64_t)b * a.Lq + qi) * a.ldo + XD * head, h);
    if (a.lse && h == 0) a.lse[(int64_t)bh * a.Lq + qi] = (m + __log2f(l)) * kLn2;
  }
}

// ------------------------------------------------------------------------------------------------ delta[b, h, i] = sum_d dout o: one wave per (row, head)
__global__ __launch_bounds__(XTHREADS) void xattn_delta_kernel(XArgs a) {
  const int64_t w = (int64_t)blockIdx.x * (XTHREADS / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= (int64_t)a.B * a.Lq * a.H) return;
  const int64_t row = w / a.H; const int head = (int)(w - row * a.H);
  const int b = (int)(row / a.Lq), i = (int)(row - (int64_t)b * a.Lq);
  const int64_t off = row * a.ldo + XD * head + 2 * lane;
  const float2 x = *reinterpret_cast<const float2*>(a.o + off), y = *reinterpret_cast<const float2*>(a.dout + off);
  const float s = wave_sum(fmaf(x.x, y.x, x.y * y.y));
  if (lane == 0) a.delta[((int64_t)b * a.H + head) * a.Lq + i] = s;
}

// ------------------------------------------------------------------------------------------------ dq
// CAUSAL (awt_op_causal_attention_backward): the forward's addressing and bounds -- k / v are the cache, the workgroup streams key tiles up to its last query's
// diagonal only (`Sk`: also the staging's valid-row count, so nothing at or past row T is loaded), a wave skips the tiles past its own last query, and inside the
// tiles that remain p = 0 where key > T - Lq + query.
template <int TERMS, bool CAUSAL = false>
__global__ __launch_bounds__(XTHREADS) void xattn_dq_kernel(XArgs a) {
  constexpr bool LO = TERMS == 3;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* kh = reinterpret_cast<bf16_t*>(smem);
  bf16_t* kl = kh + (LO ? XKT * XRP : 0);
  bf16_t* vh = kl + XKT * XRP;
  bf16_t* vl = vh + (LO ? XKT * XRP : 0);
  bf16_t* kth = vl + XKT * XRP;
  bf16_t* ktl = kth + (LO ? XD * (XKT + 8) : 0);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int nqb = (a.Lq + XLB - 1) / XLB;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb, b = bh / a.H, head = bh - b * a.H;
  const int q0 = qb * XLB + wave * XLW, qi = q0 + r;
  const bool live = q0 < a.Lq;
  const int qc = min(qi, a.Lq - 1);
  const float *kbase, *vbase;
  int Sk, lim = 0, wlim = 0;                                       // as in the forward
  if constexpr (CAUSAL) {
    const int kvh = head / (a.H / a.Hkv), off = a.Sk - a.Lq;
    kbase = a.k + (int64_t)b * a.kvbs + XD * kvh;
    vbase = a.v + (int64_t)b * a.kvbs + XD * kvh;
    Sk = off + min(qb * XLB + XLB, a.Lq);
    lim = off + qc;
    wlim = off + min(q0 + XLW, a.Lq) - 1;
  } else {
    kbase = a.k + (int64_t)b * a.Sk * a.ldk + XD * head;
    vbase = a.v + (int64_t)b * a.Sk * a.ldv + XD * head;
    Sk = a.Sk;
  }

  bf16x8 qh[8], ql[8], gh[8], gl[8];
  load_frags<LO>(a.q + ((int64_t)b * a.Lq + qc) * a.ldq + XD * head, h, qh, ql);
  load_frags<LO>(a.dout + ((int64_t)b * a.Lq + qc) * a.ldo + XD * head, h, gh, gl);
  const float lse2 = a.lse_in[(int64_t)bh * a.Lq + qc] * kLog2e, delta = a.delta_in[(int64_t)bh * a.Lq + qc];
  const float sc2 = a.scale * kLog2e;

  f32x16 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;

  const int nt = (Sk + XKT - 1) / XKT;
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * XKT;
    __syncthreads();                                               // the previous tile's fragment reads are done
    {                                                              // one image at a time: the staging registers of all three do not fit beside the fragments
      float4 kr[XKT / 8];
      load_rows<XKT>(kbase + (int64_t)k0 * a.ldk, a.ldk, Sk - k0, tid, kr);
      write_rows<XKT, LO>(kr, Sk - k0, tid, kh, kl);
    }
    {
      float4 vr[XKT / 8];
      load_rows<XKT>(vbase + (int64_t)k0 * a.ldv, a.ldv, Sk - k0, tid, vr);
      write_rows<XKT, LO>(vr, Sk - k0, tid, vh, vl);
    }
    {
      float kc[XKT / 2];
      load_cols<XKT>(kbase + (int64_t)k0 * a.ldk, a.ldk, Sk - k0, tid, kc);
      write_cols<XKT, LO>(kc, Sk - k0, tid, kth, ktl);
    }
    __syncthreads();
    if (!live) continue;
    if constexpr (CAUSAL) { if (k0 > wlim) continue; }           // wave-uniform: every key of the tile lies past this wave's last query

#pragma unroll 1
    for (int blk = 0; blk < 2; ++blk) {                            // 32 keys at a time, not unrolled: both products of a block, then the next block
      f32x16 st, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { st[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int off = (32 * blk + r) * XRP + 16 * s + 8 * h;
        st = mma3<LO>(lds_frag(kh + off), lds_frag(kl + off), qh[s], ql[s], st);
        dp = mma3<LO>(lds_frag(vh + off), lds_frag(vl + off), gh[s], gl[s], dp);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int kj = k0 + 32 * blk + acc_row(i, h);
        const float p = (CAUSAL ? kj <= lim : kj < Sk) ? __builtin_amdgcn_exp2f(fmaf(st[i], sc2, -lse2)) : 0.f;
        st[i] = p * (dp[i] - delta);
      }
      bf16x8 dsh[2], dsl[2];
      acc_frags<LO>(st, dsh, dsl);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int off = (32 * dt + r) * (XKT + 8) + 32 * blk + 16 * s + 8 * h;
          acc[dt] = mma3<LO>(lds_frag(kth + off), lds_frag(ktl + off), dsh[s], dsl[s], acc[dt]);
        }
    }
  }
  if (live && qi < a.Lq) store_acc_t(acc, a.scale, a.dq + ((int64_t)b * a.Lq + qi) * a.ldq + XD * head, h);
}

// ------------------------------------------------------------------------------------------------ dk / dv
// CAUSAL (awt_op_causal_attention_backward): one workgroup per (batch, KV head, 64-key block) of the cache.  It walks the KV head's a.H / a.Hkv query heads in
// ascending order and, per head, the 32-query tiles from the first one that can see the block's first key (query i sees key j iff j <= T - Lq + i; the tiles
// wholly before the diagonal are never loaded); dk and dv stay in the accumulators across the heads -- the group sum, in a fixed order, without atomics --
// and are stored once, in the cache's layout (a.lddkv, a.dkvbs).  p = 0 where key > T - Lq + query.
template <int TERMS, bool CAUSAL = false>
__global__ __launch_bounds__(XTHREADS) void xattn_dkv_kernel(XArgs a) {
  constexpr bool LO = TERMS == 3;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* qh = reinterpret_cast<bf16_t*>(smem);
  bf16_t* ql = qh + (LO ? XQT * XRP : 0);
  bf16_t* gh = ql + XQT * XRP;
  bf16_t* gl = gh + (LO ? XQT * XRP : 0);
  bf16_t* qth = gl + XQT * XRP;
  bf16_t* qtl = qth + (LO ? XD * (XQT + 8) : 0);
  bf16_t* gth = qtl + XD * (XQT + 8);
  bf16_t* gtl = gth + (LO ? XD * (XQT + 8) : 0);
  float* lse2_s = reinterpret_cast<float*>(gtl + XD * (XQT + 8));
  float* delta_s = lse2_s + XQT;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int nkb = (a.Sk + XKB - 1) / XKB;
  const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;     // CAUSAL: bh counts (batch, KV head) pairs
  const int nhead = CAUSAL ? a.Hkv : a.H, b = bh / nhead, head = bh - b * nhead;
  const int dh = wave & 1;                                         // this wave's half of the 128 dims: two waves share 32 keys
  const int kw0 = kb * XKB + (wave >> 1) * XLW, ki = kw0 + r;
  const bool live = kw0 < a.Sk;
  const int kc = min(ki, a.Sk - 1);

  bf16x8 kfh[8], kfl[8], vfh[8], vfl[8];
  if constexpr (CAUSAL) {                                          // the cache: batch stride kvbs, ldk = ldv
    load_frags<LO>(a.k + (int64_t)b * a.kvbs + (int64_t)kc * a.ldk + XD * head, h, kfh, kfl);
    load_frags<LO>(a.v + (int64_t)b * a.kvbs + (int64_t)kc * a.ldv + XD * head, h, vfh, vfl);
  } else {
    load_frags<LO>(a.k + ((int64_t)b * a.Sk + kc) * a.ldk + XD * head, h, kfh, kfl);
    load_frags<LO>(a.v + ((int64_t)b * a.Sk + kc) * a.ldv + XD * head, h, vfh, vfl);
  }
  const float sc2 = a.scale * kLog2e;

  f32x16 dk[2], dv[2];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[dt][i] = 0.f; dv[dt][i] = 0.f; }

  const int nt = (a.Lq + XQT - 1) / XQT;
  const int coff = a.Sk - a.Lq;                                    // CAUSAL: query i sees key j iff j <= coff + i
  const int group = CAUSAL ? a.H / a.Hkv : 1;
  const int t0 = CAUSAL ? max(kb * XKB - coff, 0) / XQT : 0;        // the first query tile that sees the block's first key (t0 < nt: key T - 1 is seen by query Lq - 1)
  int j = 0;
  do {                                                             // the KV head's query heads (non-causal: one pass, the condition below is a constant)
    const int qhead = CAUSAL ? head * group + j : head, qbh = CAUSAL ? b * a.H + qhead : bh;
    const float* qbase = a.q + (int64_t)b * a.Lq * a.ldq + XD * qhead;
    const float* gbase = a.dout + (int64_t)b * a.Lq * a.ldo + XD * qhead;
    for (int t = t0; t < nt; ++t) {
      const int q0 = t * XQT;
      __syncthreads();                                               // the previous tile's fragment reads are done
      {
        float4 qr[XQT / 8], gr[XQT / 8];
        load_rows<XQT>(qbase + (int64_t)q0 * a.ldq, a.ldq, a.Lq - q0, tid, qr);
        load_rows<XQT>(gbase + (int64_t)q0 * a.ldo, a.ldo, a.Lq - q0, tid, gr);
        write_rows<XQT, LO>(qr, a.Lq - q0, tid, qh, ql);
        write_rows<XQT, LO>(gr, a.Lq - q0, tid, gh, gl);
      }
      {
        float qc[XQT / 2], gc[XQT / 2];
        load_cols<XQT>(qbase + (int64_t)q0 * a.ldq, a.ldq, a.Lq - q0, tid, qc);
        load_cols<XQT>(gbase + (int64_t)q0 * a.ldo, a.ldo, a.Lq - q0, tid, gc);
        write_cols<XQT, LO>(qc, a.Lq - q0, tid, qth, qtl);
        write_cols<XQT, LO>(gc, a.Lq - q0, tid, gth, gtl);
      }
      if (tid < XQT) {
        const bool ok = q0 + tid < a.Lq;
        lse2_s[tid] = ok ? a.lse_in[(int64_t)qbh * a.Lq + q0 + tid] * kLog2e : 0.f;
        delta_s[tid] = ok ? a.delta_in[(int64_t)qbh * a.Lq + q0 + tid] : 0.f;
      }
      __syncthreads();
      if (!live) continue;
      if constexpr (CAUSAL) { if (coff + q0 + XQT - 1 < kw0) continue; }   // wave-uniform: no query of the tile sees any of this wave's keys
  
      f32x16 st, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { st[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int off = r * XRP + 16 * s + 8 * h;
        st = mma3<LO>(lds_frag(qh + off), lds_frag(ql + off), kfh[s], kfl[s], st);
        dp = mma3<LO>(lds_frag(gh + off), lds_frag(gl + off), vfh[s], vfl[s], dp);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, h);
        const bool seen = CAUSAL ? q0 + row < a.Lq && ki <= coff + q0 + row : q0 + row < a.Lq;
        const float p = seen ? __builtin_amdgcn_exp2f(fmaf(st[i], sc2, -lse2_s[row])) : 0.f;   // tail (and, CAUSAL, masked) queries weigh nothing
        st[i] = p;
        dp[i] = p * (dp[i] - delta_s[row]);
      }
      bf16x8 ph[2], pl[2], dsh[2], dsl[2];
      acc_frags<LO>(st, ph, pl);
      acc_frags<LO>(dp, dsh, dsl);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int off = (64 * dh + 32 * dt + r) * (XQT + 8) + 16 * s + 8 * h;
          dv[dt] = mma3<LO>(lds_frag(gth + off), lds_frag(gtl + off), ph[s], pl[s], dv[dt]);
          dk[dt] = mma3<LO>(lds_frag(qth + off), lds_frag(qtl + off), dsh[s], dsl[s], dk[dt]);
        }
    }
  } while (CAUSAL && ++j < group);
  if (live && ki < a.Sk) {
    if constexpr (CAUSAL) {
      const int64_t orow = (int64_t)b * a.dkvbs + (int64_t)ki * a.lddkv + XD * head + 64 * dh;
      store_acc_t(dk, a.scale, a.dk + orow, h);
      store_acc_t(dv, 1.0f, a.dv + orow, h);
    } else {
      store_acc_t(dk, a.scale, a.dk + ((int64_t)b * a.Sk + ki) * a.ldk + XD * head + 64 * dh, h);
      store_acc_t(dv, 1.0f, a.dv + ((int64_t)b * a.Sk + ki) * a.ldv + XD * head + 64 * dh, h);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct XWs { float* delta; size_t bytes; };
XWs xattn_layout(void* base, int B, int H, int Lq, int backward) {
  Carver cv(base);
  return {backward ? cv.take<float>((size_t)B * H * Lq * 4) : nullptr, cv.bytes()};
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_shape(const char* who, int B, int H, int Lq, int Sk, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int terms) {
  const std::string w(who);
  AWT_REQUIRE(terms == 1 || terms == 3, AWT_ERR_INVALID, w + ": terms must be 1 (bf16) or 3 (bf16x3)");
  AWT_REQUIRE(B > 0 && H > 0 && Lq > 0 && Sk > 0, AWT_ERR_INVALID, w + ": B, H, Lq and Sk must be positive");
  AWT_REQUIRE(ldq >= (int64_t)H * XD && ldk >= (int64_t)H * XD && ldv >= (int64_t)H * XD && ldo >= (int64_t)H * XD, AWT_ERR_INVALID,
              w + ": every pitch must hold H * 128 columns (head_dim is 128 in this operator)");
  AWT_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ldo % 4 == 0, AWT_ERR_INVALID, w + ": pitches must be multiples of 4");
  AWT_REQUIRE((int64_t)B * H * ((std::max(Lq, Sk) + XKB - 1) / XKB) < (1ll << 31), AWT_ERR_INVALID, w + ": too many workgroups");
  return AWT_OK;
}

}  // namespace

extern "C" size_t awt_op_cross_attention_workspace_bytes(int B, int H, int Lq, int Sk, int backward) {
  (void)Sk;
  if (B <= 0 || H <= 0 || Lq <= 0) return 0;
  return xattn_layout(nullptr, B, H, Lq, backward).bytes;
}

extern "C" int awt_op_cross_attention(awt_ctx* c, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo, float* lse,
                                      int B, int H, int Lq, int Sk, int terms, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && q && k && v && o, AWT_ERR_INVALID, "op_cross_attention: null argument");
  int rc = check_shape("op_cross_attention", B, H, Lq, Sk, ldq, ldk, ldv, ldo, terms); if (rc) return rc;
  AWT_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o), AWT_ERR_INVALID, "op_cross_attention: tensors must be 16-byte aligned");
  AWT_REQUIRE(ws_bytes >= xattn_layout(nullptr, B, H, Lq, 0).bytes, AWT_ERR_INVALID, "op_cross_attention: workspace too small");
  (void)workspace;
  XArgs a{};
  a.q = q; a.k = k; a.v = v; a.out = o; a.lse = lse; a.B = B; a.H = H; a.Lq = Lq; a.Sk = Sk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  a.scale = 0.08838834764831845f;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_ATTENTION, s, 4.0 * B * H * (double)Lq * Sk * XD * terms);
  const dim3 grid(B * H * ((Lq + XLB - 1) / XLB)), block(XTHREADS);
  return terms == 3 ? launch_kernel<xattn_fwd_kernel<3>>(grid, block, fwd_lds(3), s, a) : launch_kernel<xattn_fwd_kernel<1>>(grid, block, fwd_lds(1), s, a);
}

extern "C" int awt_op_cross_attention_backward(awt_ctx* c, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                                               const float* dout, int ldo, const float* lse, float* dq, float* dk, float* dv, int B, int H, int Lq, int Sk,
                                               int terms, void* workspace, size_t ws_bytes, void* stream) {
  AWT_REQUIRE(c && q && k && v && o && dout && lse && dq && dk && dv && workspace, AWT_ERR_INVALID, "op_cross_attention_backward: null argument");
  int rc = check_shape("op_cross_attention_backward", B, H, Lq, Sk, ldq, ldk, ldv, ldo, terms); if (rc) return rc;
  AWT_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o) && aligned16(dout) && aligned16(dq) && aligned16(dk) && aligned16(dv),
              AWT_ERR_INVALID, "op_cross_attention_backward: tensors must be 16-byte aligned");
  AWT_REQUIRE(((uintptr_t)workspace & 255) == 0, AWT_ERR_INVALID, "op_cross_attention_backward: workspace must be 256-byte aligned");
  AWT_REQUIRE(ws_bytes >= xattn_layout(nullptr, B, H, Lq, 1).bytes, AWT_ERR_INVALID, "op_cross_attention_backward: workspace too small");
  const XWs ws = xattn_layout(workspace, B, H, Lq, 1);
  XArgs a{};
  a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout; a.lse_in = lse; a.delta = ws.delta; a.delta_in = ws.delta; a.dq = dq; a.dk = dk; a.dv = dv;
  a.B = B; a.H = H; a.Lq = Lq; a.Sk = Sk; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
  a.scale = 0.08838834764831845f;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_ATTENTION_BWD, s, 10.0 * B * H * (double)Lq * Sk * XD * terms);
  const dim3 block(XTHREADS);
  const int64_t waves = (int64_t)B * Lq * H;
  hipLaunchKernelGGL(xattn_delta_kernel, dim3((unsigned)((waves + 3) / 4)), block, 0, s, a);
  AWT_HIP_CHECK(hipGetLastError());
  const dim3 gq(B * H * ((Lq + XLB - 1) / XLB)), gk(B * H * ((Sk + XKB - 1) / XKB));
  rc = terms == 3 ? launch_kernel<xattn_dq_kernel<3>>(gq, block, dq_lds(3), s, a) : launch_kernel<xattn_dq_kernel<1>>(gq, block, dq_lds(1), s, a);
  if (rc) return rc;
  return terms == 3 ? launch_kernel<xattn_dkv_kernel<3>>(gk, block, dkv_lds(3), s, a) : launch_kernel<xattn_dkv_kernel<1>>(gk, block, dkv_lds(1), s, a);
}

// ------------------------------------------------------------------------------------------------ causal self-attention over a decode cache (Qwen3Decoder)
namespace {

int check_causal(const char* who, const void* k, const void* v, int ldq, int ldkv, int64_t kv_batch_stride, int ldo, int B, int Hq, int Hkv, int Lq, int T, int terms) {
  const std::string w(who);
  AWT_REQUIRE(Hkv > 0 && Hq > 0 && Hq % Hkv == 0, AWT_ERR_INVALID, w + ": Hq must be a positive multiple of Hkv");
  AWT_REQUIRE(Lq >= 1 && T >= Lq, AWT_ERR_INVALID, w + ": needs 1 <= Lq <= T (T live cache positions, the Lq new ones included)");
  int rc = check_shape(who, B, Hq, Lq, T, ldq, ldq, ldq, ldo, terms); if (rc) return rc;   // the cache's pitch has Hkv heads: checked below
  AWT_REQUIRE(ldkv >= (int64_t)Hkv * XD && ldkv % 4 == 0, AWT_ERR_INVALID, w + ": ldkv must hold Hkv * 128 columns and be a multiple of 4");
  AWT_REQUIRE(kv_batch_stride % 4 == 0 && kv_batch_stride >= (int64_t)(T - 1) * ldkv + (int64_t)Hkv * XD, AWT_ERR_INVALID,
              w + ": kv_batch_stride must be a multiple of 4 and hold a batch's T cache rows");
  AWT_REQUIRE(aligned16(k) && aligned16(v), AWT_ERR_INVALID, w + ": tensors must be 16-byte aligned");
  return AWT_OK;
}

int causal_forward(const char* who, awt_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, int64_t kv_batch_stride, float* o, int ldo, float* lse,
                   int B, int Hq, int Hkv, int Lq, int T, int terms, size_t ws_bytes, void* stream) {
  const std::string w(who);
  AWT_REQUIRE(c && q && k && v && o, AWT_ERR_INVALID, w + ": null argument");
  int rc = check_causal(who, k, v, ldq, ldkv, kv_batch_stride, ldo, B, Hq, Hkv, Lq, T, terms); if (rc) return rc;
  AWT_REQUIRE(aligned16(q) && aligned16(o), AWT_ERR_INVALID, w + ": tensors must be 16-byte aligned");
  AWT_REQUIRE(ws_bytes >= xattn_layout(nullptr, B, Hq, Lq, 0).bytes, AWT_ERR_INVALID, w + ": workspace too small");
  XArgs a{};
  a.q = q; a.k = k; a.v = v; a.out = o; a.lse = lse; a.B = B; a.H = Hq; a.Hkv = Hkv; a.Lq = Lq; a.Sk = T; a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.ldo = ldo;
  a.kvbs = kv_batch_stride;
  a.scale = 0.08838834764831845f;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_ATTENTION, s, 2.0 * B * Hq * (double)Lq * (2.0 * T - Lq + 1) * XD * terms);   // the visible (query, key) pairs only
  const dim3 grid(B * Hq * ((Lq + XLB - 1) / XLB)), block(XTHREADS);
  return terms == 3 ? launch_kernel<xattn_fwd_kernel<3, true>>(grid, block, fwd_lds(3), s, a) : launch_kernel<xattn_fwd_kernel<1, true>>(grid, block, fwd_lds(1), s, a);
}

}  // namespace

extern "C" size_t awt_op_causal_attention_workspace_bytes(int B, int Hq, int Lq, int T) {
  (void)T;
  if (B <= 0 || Hq <= 0 || Lq <= 0) return 0;
  return xattn_layout(nullptr, B, Hq, Lq, 0).bytes;                // the forward keeps nothing outside its registers and LDS
}

extern "C" int awt_op_causal_attention(awt_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, int64_t kv_batch_stride, float* o, int ldo,
                                       int B, int Hq, int Hkv, int Lq, int T, int terms, void* workspace, size_t ws_bytes, void* stream) {
  (void)workspace;
  return causal_forward("op_causal_attention", c, q, ldq, k, v, ldkv, kv_batch_stride, o, ldo, nullptr, B, Hq, Hkv, Lq, T, terms, ws_bytes, stream);
}

extern "C" int awt_op_causal_attention_lse(awt_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, int64_t kv_batch_stride, float* o, int ldo,
                                           float* lse, int B, int Hq, int Hkv, int Lq, int T, int terms, void* workspace, size_t ws_bytes, void* stream) {
  (void)workspace;
  AWT_REQUIRE(lse, AWT_ERR_INVALID, "op_causal_attention_lse: null argument");
  return causal_forward("op_causal_attention_lse", c, q, ldq, k, v, ldkv, kv_batch_stride, o, ldo, lse, B, Hq, Hkv, Lq, T, terms, ws_bytes, stream);
}

extern "C" size_t awt_op_causal_attention_backward_workspace_bytes(int B, int Hq, int Lq, int T) {
  (void)T;
  if (B <= 0 || Hq <= 0 || Lq <= 0) return 0;
  return xattn_layout(nullptr, B, Hq, Lq, 1).bytes;                // delta [B, Hq, Lq]
}

extern "C" int awt_op_causal_attention_backward(awt_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, int64_t kv_batch_stride, const float* o,
                                                const float* dout, int ldo, const float* lse, float* dq, float* dk, float* dv, int lddkv, int64_t dkv_batch_stride,
                                                int B, int Hq, int Hkv, int Lq, int T, int terms, void* workspace, size_t ws_bytes, void* stream) {
  const char* who = "op_causal_attention_backward";
  AWT_REQUIRE(c && q && k && v && o && dout && lse && dq && dk && dv && workspace, AWT_ERR_INVALID, "op_causal_attention_backward: null argument");
  int rc = check_causal(who, k, v, ldq, ldkv, kv_batch_stride, ldo, B, Hq, Hkv, Lq, T, terms); if (rc) return rc;
  AWT_REQUIRE(lddkv >= (int64_t)Hkv * XD && lddkv % 4 == 0, AWT_ERR_INVALID, "op_causal_attention_backward: lddkv must hold Hkv * 128 columns and be a multiple of 4");
  AWT_REQUIRE(dkv_batch_stride % 4 == 0 && dkv_batch_stride >= (int64_t)(T - 1) * lddkv + (int64_t)Hkv * XD, AWT_ERR_INVALID,
              "op_causal_attention_backward: dkv_batch_stride must be a multiple of 4 and hold a batch's T rows");
  AWT_REQUIRE(aligned16(q) && aligned16(o) && aligned16(dout) && aligned16(dq) && aligned16(dk) && aligned16(dv), AWT_ERR_INVALID,
              "op_causal_attention_backward: tensors must be 16-byte aligned");
  AWT_REQUIRE(((uintptr_t)workspace & 255) == 0, AWT_ERR_INVALID, "op_causal_attention_backward: workspace must be 256-byte aligned");
  AWT_REQUIRE(ws_bytes >= xattn_layout(nullptr, B, Hq, Lq, 1).bytes, AWT_ERR_INVALID, "op_causal_attention_backward: workspace too small");
  const XWs ws = xattn_layout(workspace, B, Hq, Lq, 1);
  XArgs a{};
  a.q = q; a.k = k; a.v = v; a.o = o; a.dout = dout; a.lse_in = lse; a.delta = ws.delta; a.delta_in = ws.delta; a.dq = dq; a.dk = dk; a.dv = dv;
  a.B = B; a.H = Hq; a.Hkv = Hkv; a.Lq = Lq; a.Sk = T; a.ldq = ldq; a.ldk = ldkv; a.ldv = ldkv; a.ldo = ldo;
  a.kvbs = kv_batch_stride; a.lddkv = lddkv; a.dkvbs = dkv_batch_stride;
  a.scale = 0.08838834764831845f;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_ATTENTION_BWD, s, 5.0 * B * Hq * (double)Lq * (2.0 * T - Lq + 1) * XD * terms);   // the visible (query, key) pairs only
  const dim3 block(XTHREADS);
  const int64_t waves = (int64_t)B * Lq * Hq;
  hipLaunchKernelGGL(xattn_delta_kernel, dim3((unsigned)((waves + 3) / 4)), block, 0, s, a);
  AWT_HIP_CHECK(hipGetLastError());
  const dim3 gq(B * Hq * ((Lq + XLB - 1) / XLB)), gk(B * Hkv * ((T + XKB - 1) / XKB));
  rc = terms == 3 ? launch_kernel<xattn_dq_kernel<3, true>>(gq, block, dq_lds(3), s, a) : launch_kernel<xattn_dq_kernel<1, true>>(gq, block, dq_lds(1), s, a);
  if (rc) return rc;
  return terms == 3 ? launch_kernel<xattn_dkv_kernel<3, true>>(gk, block, dkv_lds(3), s, a) : launch_kernel<xattn_dkv_kernel<1, true>>(gk, block, dkv_lds(1), s, a);
}
