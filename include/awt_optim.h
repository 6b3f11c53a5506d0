/* awt_optim.h -- the optimizer phase of a training step on libawt.so: global-norm clipping and AdamW over any list of fp32 tensors in three
 * launches (csrc/optim.hip).  Stands behind `torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0); optimizer.step()` of the reference's
 * training loops (.charles/music2midi/train.py:498-501); `optim.FusedAdamW` wraps it.
 *
 * Why a header of its own and not a section of awt.h: tests/test_graph_capture_coverage_host.py requires every `void* stream` prototype of
 * awt.h to appear in the fixed tables of tests/graph_capture.py, and those tables belong to the tests that were written with them.  The
 * functions declared here get the same treatment from tests of their own: tests/test_optim_host.py (every declaration below is exported by
 * libawt.so and bound in _lib.py; the two queries answer without a GPU) and tests/test_gpu_optim.py (captured into a HIP graph and replayed,
 * run between canary guards, compared with float64).
 *
 * Conventions: those of awt.h.  Every pointer is a caller-owned DEVICE pointer; the one entry point enqueues on the caller's stream, never
 * synchronises, never allocates, and reads no device data on the host -- the step counters and the hyper-parameters live on the device -- so
 * it can be captured into a HIP graph, and every replay is one more optimizer step.
 */
#ifndef AWT_OPTIM_H_
#define AWT_OPTIM_H_

#include "awt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One tensor of the step: parameter, gradient, first and second moment (n fp32 elements each, any 4-byte alignment, each on its own), the
 * hyper-parameter group it belongs to and the slot of its step counter.  No two tensors of a table may overlap. */
typedef struct awt_optim_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  int32_t group;
  int32_t index;
} awt_optim_tensor;

typedef struct awt_optim_group {
  float lr, weight_decay, beta1, beta2, eps, pad[3];
} awt_optim_group;

/* Elements one workgroup handles.  A tensor of n elements takes ceil(n / chunk) chunks; a chunk never spans two tensors. */
int awt_optim_chunk_elems(void);
/* Workspace of a step over `chunks` chunks in all (one partial sum per chunk, two bias corrections per tensor; a table has no more tensors
 * than chunks). */
size_t awt_op_adamw_workspace_bytes(int64_t chunks);

/* clip_grad_norm_(max_norm, error_if_nonfinite=False) followed by torch.optim.AdamW(amsgrad=False, maximize=False).step(), without
 * modifying the gradients:
 *   norm = sqrt(sum over every listed tensor of g^2);  coef = min(1, max_norm / (norm + 1e-6)), or 1 when max_norm <= 0 or infinite
 *   per tensor: t = steps[index] += 1;  bc1 = 1 - beta1^t;  bc2 = 1 - beta2^t                       (float64)
 *   per element: g' = g coef;  p *= 1 - lr wd;  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2;
 *                p -= (lr / bc1) (m / (sqrt(v) / sqrt(bc2) + eps))
 * tensors      device [T]; first_chunk device int32 [T + 1]: first_chunk[0] = 0, first_chunk[t + 1] = first_chunk[t] + ceil(n_t / chunk),
 *              first_chunk[T] = chunks.  T >= 1, every n >= 1.
 * groups       device [G]; steps: device float [P], one counter per parameter (torch keeps `step` as a float32 tensor too).
 * norm_out     device float [2]: the total norm (produced whether or not it clips) and the coefficient applied.
 * workspace    >= awt_op_adamw_workspace_bytes(chunks) bytes, 256-byte aligned.
 * Three launches whatever T is, no atomics: two runs on the same bits give the same bits.  A non-finite gradient behaves as it does in torch:
 * an inf makes coef 0 and its own element NaN, a NaN makes coef NaN and every element of every tensor NaN. */
int awt_op_adamw_step(awt_ctx* c, const awt_optim_tensor* tensors, const int32_t* first_chunk, int T, int64_t chunks,
                      const awt_optim_group* groups, int G, float* steps, float max_norm, float* norm_out,
                      void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AWT_OPTIM_H_ */
