// The optimizer phase of a training step (include/awt_optim.h): global-norm clipping + AdamW over a table of fp32 tensors.
//   awt_op_adamw_step     three launches whatever the number of tensors:
//     adamw_sumsq_kernel     one workgroup per chunk of OPT_CHUNK elements: sum of g^2 in fp32, a fixed order, one partial per chunk
//     adamw_finalize_kernel  one workgroup: the partials in index order in fp64 -> norm and clip coefficient; every tensor's step counter + 1 and its
//                            two bias corrections in fp64
//     adamw_update_kernel    one workgroup per chunk: p, m, v updated in place from g (read only): 16 bytes read and 12 written per element
// A workgroup finds its (tensor, offset) by a binary search of the chunk table, so the launch count does not depend on the table.  16-byte accesses where
// every pointer of the tensor is 16-byte aligned (a chunk starts a multiple of 4 elements into its tensor), 4-byte ones elsewhere and in a tensor's last
// n % 4 elements: the element -> (thread, order) assignment is the same in both forms, so the bits do not depend on the alignment either.  No atomics.
// The element arithmetic is written one rounding per operation, in the order torch.optim.AdamW's tensor operations round (no contraction into FMAs, IEEE
// division and square root), so that it differs from an fp32 restatement of the step only through the clip coefficient.
#include "common.h"
#include "../../include/awt_optim.h"

#pragma clang fp contract(off)

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = 8192;                              // elements per workgroup: 8 groups of 4 = 32 elements per thread
constexpr int OPT_ITERS = OPT_CHUNK / (OPT_THREADS * 4);     // groups of 4 per thread
constexpr int OPT_UNROLL = 4;                                // full chunks: the loads of 4 groups are issued before the first is used
static_assert(OPT_CHUNK % (OPT_THREADS * 4 * OPT_UNROLL) == 0, "a chunk is a whole number of unrolled rounds");

struct OptWs { float* partials; double* bc; size_t bytes; };
OptWs optim_layout(void* base, int64_t chunks) {
  Carver cv(base);
  float* partials = cv.take<float>((size_t)chunks * sizeof(float));
  double* bc = cv.take<double>((size_t)chunks * 2 * sizeof(double));     // per tensor: 1 - beta1^t, sqrt(1 - beta2^t); T <= chunks
  return {partials, bc, cv.bytes()};
}

__device__ __forceinline__ bool aligned16d(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the tensor of chunk `b`: the last t with first_chunk[t] <= b (first_chunk[0] = 0, first_chunk[T] = chunks > b)
__device__ __forceinline__ int find_tensor(const int32_t* __restrict__ first_chunk, int T, int b) {
  int lo = 0, hi = T;                                        // invariant: first_chunk[lo] <= b < first_chunk[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first_chunk[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_sumsq_kernel(const awt_optim_tensor* __restrict__ tensors, const int32_t* __restrict__ first_chunk, int T,
                                                                  float* __restrict__ partials) {
  __shared__ float wave_part[OPT_THREADS / AWT_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int t = find_tensor(first_chunk, T, b);
  const awt_optim_tensor ten = tensors[t];
  const int64_t off = (int64_t)(b - first_chunk[t]) * OPT_CHUNK;
  const int64_t left = ten.n - off;
  const int len = left < OPT_CHUNK ? (left > 0 ? (int)left : 0) : OPT_CHUNK;
  const float* g = ten.g + off;
  const bool vec = aligned16d(ten.g);
  float acc = 0.f;
  if (vec && len == OPT_CHUNK) {
#pragma unroll
    for (int it = 0; it < OPT_ITERS; ++it) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(g + (it * OPT_THREADS + tid) * 4);
      acc = acc + x[0] * x[0]; acc = acc + x[1] * x[1]; acc = acc + x[2] * x[2]; acc = acc + x[3] * x[3];
    }
  } else {
    for (int it = 0; it < OPT_ITERS; ++it) {
      const int e = (it * OPT_THREADS + tid) * 4;
      if (e >= len) break;
      if (vec && e + 4 <= len) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(g + e);
        acc = acc + x[0] * x[0]; acc = acc + x[1] * x[1]; acc = acc + x[2] * x[2]; acc = acc + x[3] * x[3];
      } else {
        for (int k = 0; k < 4 && e + k < len; ++k) { const float x = g[e + k]; acc = acc + x * x; }
      }
    }
  }
  acc = wave_sum(acc);
  if ((tid & (AWT_WAVE - 1)) == 0) wave_part[tid / AWT_WAVE] = acc;
  __syncthreads();
  if (tid == 0) partials[b] = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_finalize_kernel(const float* __restrict__ partials, int64_t chunks, const awt_optim_tensor* __restrict__ tensors,
                                                                     int T, const awt_optim_group* __restrict__ groups, int G, float* __restrict__ steps,
                                                                     float max_norm, float* __restrict__ norm_out, double* __restrict__ bc) {
  __shared__ double run[OPT_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = (chunks + OPT_THREADS - 1) / OPT_THREADS;          // thread i owns partials [i per, (i + 1) per): index order within and across threads
  const int64_t b0 = tid * per, b1 = b0 + per < chunks ? b0 + per : chunks;
  double s = 0.0;
  for (int64_t i = b0; i < b1; ++i) s += (double)partials[i];
  run[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int i = 0; i < OPT_THREADS; ++i) total += run[i];
    const float norm = (float)sqrt(total);
    float coef = 1.f;
    if (max_norm > 0.f && max_norm <= 3.402823466e38f) {
      const float c = max_norm / (norm + 1e-6f);
      coef = c > 1.f ? 1.f : c;                                          // a NaN norm stays a NaN coefficient, as torch.clamp(max=1) leaves it
    }
    norm_out[0] = norm;
    norm_out[1] = coef;
  }
  for (int i = tid; i < T; i += OPT_THREADS) {
    const awt_optim_tensor ten = tensors[i];
    if (ten.group < 0 || ten.group >= G) continue;
    const awt_optim_group h = groups[ten.group];
    const float t = steps[ten.index] + 1.f;
    steps[ten.index] = t;
    bc[2 * i] = 1.0 - pow((double)h.beta1, (double)t);
    bc[2 * i + 1] = sqrt(1.0 - pow((double)h.beta2, (double)t));
  }
}

struct Hyper { float coef, decay, omb1, beta2, omb2, bc2s, eps, step; };

__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const Hyper& h) {
  const float gs = g * h.coef;
  p = p * h.decay;
  m = m + (gs - m) * h.omb1;
  v = h.beta2 * v + h.omb2 * (gs * gs);
  const float denom = sqrtf(v) / h.bc2s + h.eps;
  p = p - h.step * (m / denom);
}

__device__ __forceinline__ void adamw_group4(float* p, const float* g, float* m, float* v, const Hyper& h) {
  f32x4 P = *reinterpret_cast<const f32x4*>(p), M = *reinterpret_cast<const f32x4*>(m), V = *reinterpret_cast<const f32x4*>(v);
  const f32x4 Gv = *reinterpret_cast<const f32x4*>(g);
#pragma unroll
  for (int k = 0; k < 4; ++k) { float pk = P[k], mk = M[k], vk = V[k]; adamw_element(pk, Gv[k], mk, vk, h); P[k] = pk; M[k] = mk; V[k] = vk; }
  *reinterpret_cast<f32x4*>(p) = P; *reinterpret_cast<f32x4*>(m) = M; *reinterpret_cast<f32x4*>(v) = V;
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_update_kernel(const awt_optim_tensor* __restrict__ tensors, const int32_t* __restrict__ first_chunk, int T,
                                                                   const awt_optim_group* __restrict__ groups, int G, const float* __restrict__ norm_out,
                                                                   const double* __restrict__ bc) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int t = find_tensor(first_chunk, T, b);
  const awt_optim_tensor ten = tensors[t];
  if (ten.group < 0 || ten.group >= G) return;                           // workgroup-uniform
  const awt_optim_group hp = groups[ten.group];
  Hyper h;
  h.coef = norm_out[1];
  h.decay = (float)(1.0 - (double)hp.lr * (double)hp.weight_decay);
  h.omb1 = (float)(1.0 - (double)hp.beta1);
  h.beta2 = hp.beta2;
  h.omb2 = (float)(1.0 - (double)hp.beta2);
  h.bc2s = (float)bc[2 * t + 1];
  h.eps = hp.eps;
  h.step = (float)((double)hp.lr / bc[2 * t]);
  const int64_t off = (int64_t)(b - first_chunk[t]) * OPT_CHUNK;
  const int64_t left = ten.n - off;
  const int len = left < OPT_CHUNK ? (left > 0 ? (int)left : 0) : OPT_CHUNK;
  float* p = ten.p + off; const float* g = ten.g + off; float* m = ten.m + off; float* v = ten.v + off;
  const bool vec = aligned16d(ten.p) && aligned16d(ten.g) && aligned16d(ten.m) && aligned16d(ten.v);
  if (vec && len == OPT_CHUNK) {
    for (int it = 0; it < OPT_ITERS; it += OPT_UNROLL) {
      f32x4 P[OPT_UNROLL], Gv[OPT_UNROLL], M[OPT_UNROLL], V[OPT_UNROLL];
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int e = ((it + u) * OPT_THREADS + tid) * 4;
        P[u] = *reinterpret_cast<const f32x4*>(p + e); Gv[u] = *reinterpret_cast<const f32x4*>(g + e);
        M[u] = *reinterpret_cast<const f32x4*>(m + e); V[u] = *reinterpret_cast<const f32x4*>(v + e);
      }
#pragma unroll
      for (int u = 0; u < OPT_UNROLL; ++u) {
        const int e = ((it + u) * OPT_THREADS + tid) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) { float pk = P[u][k], mk = M[u][k], vk = V[u][k]; adamw_element(pk, Gv[u][k], mk, vk, h); P[u][k] = pk; M[u][k] = mk; V[u][k] = vk; }
        *reinterpret_cast<f32x4*>(p + e) = P[u]; *reinterpret_cast<f32x4*>(m + e) = M[u]; *reinterpret_cast<f32x4*>(v + e) = V[u];
      }
    }
    return;
  }
  for (int it = 0; it < OPT_ITERS; ++it) {
    const int e = (it * OPT_THREADS + tid) * 4;
    if (e >= len) break;
    if (vec && e + 4 <= len) {
      adamw_group4(p + e, g + e, m + e, v + e, h);
    } else {
      for (int k = 0; k < 4 && e + k < len; ++k) {
        float pk = p[e + k], mk = m[e + k], vk = v[e + k];
        adamw_element(pk, g[e + k], mk, vk, h);
        p[e + k] = pk; m[e + k] = mk; v[e + k] = vk;
      }
    }
  }
}

}  // namespace

extern "C" int awt_optim_chunk_elems(void) { return OPT_CHUNK; }

extern "C" size_t awt_op_adamw_workspace_bytes(int64_t chunks) { return chunks > 0 ? optim_layout(nullptr, chunks).bytes : 0; }

extern "C" int awt_op_adamw_step(awt_ctx* c, const awt_optim_tensor* tensors, const int32_t* first_chunk, int T, int64_t chunks, const awt_optim_group* groups, int G,
                                 float* steps, float max_norm, float* norm_out, void* workspace, size_t workspace_bytes, void* stream) {
  AWT_REQUIRE(c && tensors && first_chunk && groups && steps && norm_out && workspace, AWT_ERR_INVALID, "op_adamw_step: null argument");
  AWT_REQUIRE(T > 0 && G > 0 && chunks >= T && chunks <= 0x7fffffff, AWT_ERR_INVALID,
              "op_adamw_step: T and G must be positive and chunks in [T, 2^31 - 1] (every tensor has at least one chunk)");
  AWT_REQUIRE(max_norm == max_norm, AWT_ERR_INVALID, "op_adamw_step: max_norm is NaN (<= 0 or infinity switch clipping off)");
  AWT_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)tensors & 7) == 0 && ((uintptr_t)first_chunk & 3) == 0 && ((uintptr_t)groups & 3) == 0 &&
              ((uintptr_t)steps & 3) == 0 && ((uintptr_t)norm_out & 3) == 0, AWT_ERR_INVALID,
              "op_adamw_step: the workspace must be 256-byte aligned, the tensor table 8-byte, every other table 4-byte");
  const OptWs ws = optim_layout(workspace, chunks);
  AWT_REQUIRE(workspace_bytes >= ws.bytes, AWT_ERR_WORKSPACE, "op_adamw_step: workspace smaller than awt_op_adamw_workspace_bytes(chunks)");
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(c, AWT_PROF_OTHER, s);
  hipLaunchKernelGGL(adamw_sumsq_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, s, tensors, first_chunk, T, ws.partials);
  AWT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(adamw_finalize_kernel, dim3(1), dim3(OPT_THREADS), 0, s, (const float*)ws.partials, chunks, tensors, T, groups, G, steps, max_norm, norm_out, ws.bc);
  AWT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(adamw_update_kernel, dim3((unsigned)chunks), dim3(OPT_THREADS), 0, s, tensors, first_chunk, T, groups, G, (const float*)norm_out,
                     (const double*)ws.bc);
  AWT_HIP_CHECK(hipGetLastError());
  return AWT_OK;
}
