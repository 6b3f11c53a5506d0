// Launchers of the full-parameter backward (wgrad.hip, decoder_ops.hip): weight-gradient GEMM, bias / LayerNorm parameter reductions.
#pragma once
#include "common.h"

// a row-major bf16 plane pair [rows, ld]; the operand is columns col .. col + width - 1 (lo null: one bf16 product)
struct WgradOperand { const bf16_t* hi; const bf16_t* lo; int64_t ld; int col; };
// X row of contraction row m: (m / rows_out) * rows_in + (m % rows_out) * row_mul + row_add, zero outside [0, rows_in) of its group
// (GemmSeg's row map: conv2's taps read row 2 s + tap - 1 of the conv1 output)
struct WgradRowMap { int rows_out, rows_in, row_mul, row_add; };

// out[n sn + k sk] (+)= scale * sum_m Y[m, y.col + n] X[map(m), x.col + k]   for n < N, k < K; N, K, pitches, offsets: multiples of 8.
// Two launches (slab partials, then their sum in slab order): deterministic.  partial: >= wgrad_partial_bytes(M, N, K) bytes.
int launch_wgrad(awt_ctx* c, const WgradOperand& y, int N, const WgradOperand& x, int K, int M, const WgradRowMap* map, int terms, float scale,
                 float* out, int64_t sn, int64_t sk, int accumulate, float* partial, size_t partial_bytes, hipStream_t s);
int wgrad_slabs(int M, int N, int K, int* slab_rows);       // slabs M is cut into: a function of the shape only
size_t wgrad_partial_bytes(int M, int N, int K);
// planes of dy * gelu'(pre), n elements (a multiple of 4)
int launch_dgelu_planes(awt_ctx* c, const float* dy, const float* pre, int64_t n, const PlanePair& out, hipStream_t s);
// dst [N, C] = src[:, :, tap] of a Conv1d weight [N, C, 3]
int launch_conv_tap(awt_ctx* c, const float* src, int N, int C, int tap, float* dst, hipStream_t s);

// Column reductions over M rows (decoder_ops.hip, the row kernels behind awt_op_column_sums / awt_op_layernorm_param_grad):
//   dbeta[c] (+)= scale * sum_m g[m, c],   dgamma[c] (+)= scale * sum_m g[m, c] xhat[m, c]   (x null: dbeta only)
// with g either fp32 rows `dy` [M, d] or the plane pair dyp of pitch ld (its first d columns); d <= 1280.
// partial: >= param_grad_partial_bytes(M, d) bytes.
size_t param_grad_partial_bytes(int M, int d);
int launch_param_grad(awt_ctx* c, const float* dy, const PlanePair& dyp, int64_t ld, const float* x, int M, int d, float eps,
                      float scale, int accumulate, float* dgamma, float* dbeta, float* partial, hipStream_t s);
