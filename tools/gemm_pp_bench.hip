// Standalone bring-up / timing harness of the persistent ping-pong GEMM K-loop (csrc/gemm_pp.h).  GPU box only.
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 tools/gemm_pp_bench.hip -o tools/_bin/gemm_pp_bench [-L... -lawt for the A/B leg]
//   tools/_bin/gemm_pp_bench [check|time|cus|ab|all] [M]
// Data are a hash of the element index (bit-identical on host and device), the reference is fp64 on the host over sampled outputs.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <algorithm>
#include "../mlx8-ws-audio-transformer_amd/csrc/gemm_pp.h"

void awt_set_error(const std::string&) {}
int awt_fail(int code, const std::string& m) { fprintf(stderr, "awt_fail: %s\n", m.c_str()); return code; }

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr int kKTile = 32, kElemBytes = 4;   // K per K-tile (64 per X + Y pair of 128-byte lines), operand bytes per element (fp16 + two e4m3)

__host__ __device__ inline unsigned hash32(unsigned x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; }
// ~N(0, 1): four exact 16-bit uniforms, one rounding
__host__ __device__ inline float gen(unsigned seed, unsigned long long i) {
  const unsigned a = hash32((unsigned)i * 2654435761U + seed), b = hash32(a + (unsigned)(i >> 32) + 0x9e3779b9U);
  const float u = (float)(a & 0xFFFF) + (float)(a >> 16) + (float)(b & 0xFFFF) + (float)(b >> 16);
  return (u * (1.0f / 65536.0f) - 2.0f) * 1.7320508f;
}

// ---- operand packing (device)
__global__ void pack_a_split(char* A, int M, int K, unsigned seed) {   // split lines [M][K / 64][fp16 x 64 | hi8 x 64 | lo8 x 64]
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)M * K / 4) return;
  const long long e = i * 4; const int m = (int)(e / K), k = (int)(e % K), grp = k >> 6, kk = k & 63;
  float v[4];
  for (int t = 0; t < 4; ++t) v[t] = gen(seed, e + t);
  uint2 h16; unsigned hi8, lo8;
  f16f8x4<kF8Act>(v, h16, hi8, lo8);
  char* line = A + ((long long)m * (K / 64) + grp) * 256;
  *reinterpret_cast<uint2*>(line + kk * 2) = h16;
  *reinterpret_cast<unsigned*>(line + 128 + kk) = hi8;
  *reinterpret_cast<unsigned*>(line + 192 + kk) = lo8;
}
__global__ void pack_w(char* W, int N, int Npad, int K, unsigned seed, float scale) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)Npad * K / 4) return;
  const long long e = i * 4; const int n = (int)(e / K), k = (int)(e % K), nk = K / kKTile;
  float v[4];
  for (int t = 0; t < 4; ++t) v[t] = n < N ? gen(seed, (long long)n * K + k + t) * scale : 0.0f;
  const int bn = n >> 8, nin = n & 255, s = (nin >> 5) & 1;
  // 64-deep groups: fp16 into the X K-tile 2 grp (chunk = kk / 8), lo8 | hi8 into the Y K-tile 2 grp + 1 (chunks kk / 16, 4 + kk / 16)
  const int grp = k >> 6, k6 = k & 63;
  uint2 h16; unsigned hi8, lo8;
  f16f8x4<kF8Wgt>(v, h16, hi8, lo8);
  char* rx = W + pp::w_region_offset(bn, 2 * grp, s, nk);
  char* ry = W + pp::w_region_offset(bn, 2 * grp + 1, s, nk);
  *reinterpret_cast<uint2*>(rx + pp::w_row_offset(nin, k6 >> 3) + (k6 & 7) * 2) = h16;
  *reinterpret_cast<unsigned*>(ry + pp::w_row_offset(nin, k6 >> 4) + (k6 & 15)) = lo8;
  *reinterpret_cast<unsigned*>(ry + pp::w_row_offset(nin, 4 + (k6 >> 4)) + (k6 & 15)) = hi8;
}

// ---- test kernels: EPI 0 = no epilogue (accumulators kept alive), 1 = fp32 C straight from the accumulator layout, 2 = as 0 with clock stamps
struct TestOut { float* C; long long ldc; int M, N; unsigned long long* stamps; };
template <int EPI>
__global__ __launch_bounds__(512, 2) void gemm_pp_test(pp::Args g, TestOut o) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wr = wave >> 2, wc = wave & 3;
  unsigned long long t0 = 0, r0 = 0;
  if constexpr (EPI == 2) { t0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); }
  pp::kloop(g, smem, [&](int tm, int tn, pp::Acc& accs) {
    auto& acc = accs.t;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += acc[i][j][r];
    if (s == 123.456f) o.C[0] = s;
    if constexpr (EPI == 1) {   // 16 x 16 tiles: C/D col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = tm * 256 + wr * 128 + i * 16 + (lane >> 4) * 4 + r, n = tn * 256 + wc * 64 + j * 16 + (lane & 15);
            if (m < o.M && n < o.N) o.C[(long long)m * o.ldc + n] = acc[i][j][r];
          }
    }
  });
  if constexpr (EPI == 2) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { o.stamps[blockIdx.x * 2] = t1 - t0; o.stamps[blockIdx.x * 2 + 1] = r1 - r0; }
  }
}

struct Problem { const char* name; int M, N, K; };

template <int EPI>
static float run(const Problem& p, char* A, char* W, float* C, int reps, int grid_limit = 256, unsigned long long* stamps = nullptr) {
  pp::Args g{};
  g.A = A; g.a_row_bytes = (long long)p.K * kElemBytes; g.W = W;
  g.M = p.M; g.N = p.N; g.K = p.K; g.nk = p.K / kKTile;
  g.tiles_m = (p.M + 255) / 256; g.tiles_n = (p.N + 255) / 256; g.ntiles = g.tiles_m * g.tiles_n; g.gm = 8;
  TestOut o{C, p.N, p.M, p.N, stamps};
  const int grid = g.ntiles < grid_limit ? g.ntiles : grid_limit;
  static bool attr_set = false;
  if (!attr_set) { CK(hipFuncSetAttribute((const void*)gemm_pp_test<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, pp::LDS_BYTES)); attr_set = true; }
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipLaunchKernelGGL((gemm_pp_test<EPI>), dim3(grid), dim3(512), pp::LDS_BYTES, 0, g, o);   // warm-up
  CK(hipGetLastError());
  CK(hipEventRecord(e0));
  for (int r = 0; r < reps; ++r) hipLaunchKernelGGL((gemm_pp_test<EPI>), dim3(grid), dim3(512), pp::LDS_BYTES, 0, g, o);
  CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
  float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  return ms / reps;
}

static void prepare(const Problem& p, char*& A, char*& W, unsigned seed) {
  const int Npad = (p.N + 255) / 256 * 256;
  const int Mpad = (p.M + 255) / 256 * 256;        // the kernel reads whole 256-row panels (rows >= M are never stored)
  const size_t ab = (size_t)Mpad * p.K * kElemBytes, wbytes = (size_t)Npad * p.K * kElemBytes;
  CK(hipMalloc(&A, ab)); CK(hipMalloc(&W, wbytes));
  CK(hipMemset(A, 0, ab));
  const long long na = (long long)p.M * p.K / 4, nw = (long long)Npad * p.K / 4;
  hipLaunchKernelGGL(pack_a_split, dim3((na + 255) / 256), dim3(256), 0, 0, A, p.M, p.K, seed);
  hipLaunchKernelGGL(pack_w, dim3((nw + 255) / 256), dim3(256), 0, 0, W, p.N, Npad, p.K, seed + 1, 1.0f / sqrtf((float)p.K));
  CK(hipDeviceSynchronize());
}

static bool check(const Problem& p, int grid_limit) {
  char *A, *W; float* C;
  prepare(p, A, W, 1234);
  CK(hipMalloc(&C, (size_t)p.M * p.N * 4));
  CK(hipMemset(C, 0xFF, (size_t)p.M * p.N * 4));
  run<1>(p, A, W, C, 1, grid_limit);
  std::vector<float> h((size_t)p.M * p.N);
  CK(hipMemcpy(h.data(), C, h.size() * 4, hipMemcpyDeviceToHost));
  const float ws = 1.0f / sqrtf((float)p.K);
  double worst = 0; int bad = 0; long long nsamp = 0;
  const int step_m = p.M > 4096 ? 97 : 1, step_n = p.M > 4096 ? 13 : 1;
  for (int m = 0; m < p.M; m += step_m)
    for (int n = (m * 7) % step_n; n < p.N; n += step_n) {
      double ref = 0;
      for (int k = 0; k < p.K; ++k) ref += (double)gen(1234, (long long)m * p.K + k) * (double)(gen(1235, (long long)n * p.K + k) * ws);
      const double err = fabs((double)h[(size_t)m * p.N + n] - ref);
      if (!(err <= 3e-4)) { if (bad < 8) printf("  bad m=%d n=%d got %.6f ref %.6f\n", m, n, h[(size_t)m * p.N + n], ref); ++bad; }
      if (err > worst || err != err) worst = err;
      ++nsamp;
    }
  printf("check %-6s M=%d N=%d K=%d grid<=%d: %lld samples, max|err| %.3e, bad %d\n", p.name, p.M, p.N, p.K, grid_limit, nsamp, worst, bad);
  CK(hipFree(A)); CK(hipFree(W)); CK(hipFree(C));
  return bad == 0;
}

static void timing(const Problem& p, int reps) {
  char *A, *W; float* C;
  prepare(p, A, W, 99);
  CK(hipMalloc(&C, (size_t)p.M * p.N * 4));
  const double fl = 2.0 * p.M * p.N * p.K;
  const float t0 = run<0>(p, A, W, C, reps), t1 = run<1>(p, A, W, C, reps);
  const float t0b = run<0>(p, A, W, C, reps), t1b = run<1>(p, A, W, C, reps);
  // in-kernel clock and cycles per K-tile (stamps around the whole persistent loop only; median workgroup)
  unsigned long long* st; CK(hipMalloc(&st, 256 * 16)); CK(hipMemset(st, 0, 256 * 16));
  const float t2 = run<2>(p, A, W, C, reps, 256, st);
  std::vector<unsigned long long> hs(512); CK(hipMemcpy(hs.data(), st, 256 * 16, hipMemcpyDeviceToHost)); CK(hipFree(st));
  std::vector<double> cyc, clk;
  const int ntiles = ((p.M + 255) / 256) * ((p.N + 255) / 256), nkt = p.K / kKTile;
  for (int b = 0; b < 256 && b < ntiles; ++b) {
    const int nmine = (ntiles - b + 255) / 256;
    cyc.push_back((double)hs[2 * b] / ((double)nmine * nkt)); clk.push_back((double)hs[2 * b] / (double)hs[2 * b + 1] * 0.1);
  }
  std::sort(cyc.begin(), cyc.end()); std::sort(clk.begin(), clk.end());
  printf("time  %-6s M=%d N=%d K=%d: no-epilogue %.3f / %.3f ms (%.0f TFLOP/s)   fp32-store %.3f / %.3f ms (%.0f TFLOP/s)   stamped %.3f ms: %.0f cycles per K-tile (2048 = matrix pipe saturated), clock %.2f GHz (medians)\n", p.name, p.M, p.N, p.K,
         t0, t0b, fl / (t0b < t0 ? t0b : t0) / 1e9, t1, t1b, fl / (t1b < t1 ? t1b : t1) / 1e9, t2, cyc[cyc.size() / 2], clk[clk.size() / 2]);
  fflush(stdout);
  CK(hipFree(A)); CK(hipFree(W)); CK(hipFree(C));
}

// ---- A/B against the shipped library kernel (awt_op_linear, f16f8, fp32 output), interleaved rounds in this process
__global__ void fill_f32(float* x, long long n, unsigned seed, float scale) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = gen(seed, i) * scale;
}
struct Awt {
  void* h = nullptr; void* ctx = nullptr;
  int (*ctx_create)(int, void**) = nullptr;
  int (*op_linear)(void*, const float*, const float*, const float*, float*, int, int, int, int, void*, size_t, void*) = nullptr;
  size_t (*ws_bytes)(int, int, int) = nullptr;
  int (*prof_enable)(void*, int) = nullptr;
  int (*prof_collect)(void*, int, double*, long long*, double*) = nullptr;
  bool open() {
    h = dlopen("mlx8-ws-audio-transformer_amd/libawt.so", RTLD_NOW);
    if (!h) { printf("dlopen libawt.so failed: %s\n", dlerror()); return false; }
    ctx_create = (decltype(ctx_create))dlsym(h, "awt_ctx_create"); op_linear = (decltype(op_linear))dlsym(h, "awt_op_linear");
    ws_bytes = (decltype(ws_bytes))dlsym(h, "awt_op_linear_workspace_bytes"); prof_enable = (decltype(prof_enable))dlsym(h, "awt_prof_enable");
    prof_collect = (decltype(prof_collect))dlsym(h, "awt_prof_collect");
    return ctx_create && op_linear && ws_bytes && prof_enable && prof_collect && ctx_create(0, &ctx) == 0;
  }
};
static void ab(Awt& L, const Problem& p, int rounds) {
  char *A, *W; float *C, *x, *w; void* ws;
  prepare(p, A, W, 99);
  CK(hipMalloc(&C, (size_t)p.M * p.N * 4)); CK(hipMalloc(&x, (size_t)p.M * p.K * 4)); CK(hipMalloc(&w, (size_t)p.N * p.K * 4));
  const size_t wsb = L.ws_bytes(p.M, p.N, p.K); CK(hipMalloc(&ws, wsb));
  hipLaunchKernelGGL(fill_f32, dim3(((long long)p.M * p.K + 255) / 256), dim3(256), 0, 0, x, (long long)p.M * p.K, 99u, 1.0f);
  hipLaunchKernelGGL(fill_f32, dim3(((long long)p.N * p.K + 255) / 256), dim3(256), 0, 0, w, (long long)p.N * p.K, 100u, 1.0f / sqrtf((float)p.K));
  CK(hipDeviceSynchronize());
  const double fl = 2.0 * p.M * p.N * p.K;
  double best_old = 1e9, best_new = 1e9, sum_old = 0, sum_new = 0;
  for (int r = 0; r < rounds; ++r) {
    L.prof_enable(L.ctx, 1 << 1);
    double ms = 0, f = 0; long long cnt = 0;
    L.prof_collect(L.ctx, 1, &ms, &cnt, &f);
    for (int i = 0; i < 3; ++i) if (L.op_linear(L.ctx, x, w, nullptr, C, p.M, p.N, p.K, 5, ws, wsb, nullptr) != 0) { printf("op_linear failed\n"); return; }
    L.prof_collect(L.ctx, 1, &ms, &cnt, &f); L.prof_enable(L.ctx, 0);
    const double told = ms / (cnt ? cnt : 1);
    const double tnew = run<1>(p, A, W, C, 3);
    best_old = told < best_old ? told : best_old; best_new = tnew < best_new ? tnew : best_new; sum_old += told; sum_new += tnew;
  }
  printf("ab    %-6s M=%d N=%d K=%d f16f8 fp32-out: shipped %.3f ms mean / %.3f best (%.0f TF)   ping-pong %.3f mean / %.3f best (%.0f TF)   ratio %.3f\n", p.name, p.M, p.N, p.K,
         sum_old / rounds, best_old, fl / best_old / 1e9, sum_new / rounds, best_new, fl / best_new / 1e9, sum_new / sum_old);
  fflush(stdout);
  CK(hipFree(A)); CK(hipFree(W)); CK(hipFree(C)); CK(hipFree(x)); CK(hipFree(w)); CK(hipFree(ws));
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "all";
  const int M = argc > 2 ? atoi(argv[2]) : 96000;
  bool ok = true;
  if (mode == "check" || mode == "all") {
    const Problem small[] = {{"s1", 256, 256, 256}, {"s2", 512, 768, 256}, {"s3", 1000, 512, 768}, {"s4", 2304, 768, 384}};
    for (const auto& p : small) {
      ok &= check(p, 256);
      ok &= check(p, 2);      // few workgroups: several tiles per workgroup (the continuous K-tile stream across tile boundaries)
    }
    const Problem big = {"qkv", 24000, 2304, 768};
    ok &= check(big, 256);
    printf(ok ? "CHECK OK\n" : "CHECK FAILED\n");
    if (!ok) return 1;
  }
  if (mode == "time" || mode == "all") {
    const Problem shapes[] = {{"qkv", M, 2304, 768}, {"out", M, 768, 768}, {"fc1", M, 3072, 768}, {"fc2", M, 768, 3072}};
    for (const auto& p : shapes) timing(p, 10);
    const Problem cube = {"4k", 4096, 4096, 4096}, cube8 = {"8k", 8192, 8192, 8192};
    timing(cube, 10); timing(cube8, 5);
  }
  if (mode == "cus") {   // is the exposed store time a per-CU limit or a chip-wide (HBM) one?  The same GEMM on 256 / 128 / 64 persistent workgroups
    const Problem p = {"fc1", M, 3072, 768};
    char *A, *W; float* C;
    prepare(p, A, W, 99);
    CK(hipMalloc(&C, (size_t)p.M * p.N * 4));
    const int ntiles = ((p.M + 255) / 256) * (p.N / 256);
    for (int grid : {256, 128, 64, 32}) {
      const float t0 = run<0>(p, A, W, C, 5, grid), t1 = run<1>(p, A, W, C, 5, grid);
      const double tiles_per_wg = (double)ntiles / grid;
      printf("cus   fc1 on %3d workgroups: K loops only %.3f ms, with fp32 stores %.3f ms -> %.2f us of exposed store time per 256 KB tile = %.1f GB/s per CU, %.2f TB/s chip-wide\n", grid, t0, t1,
             (t1 - t0) * 1e3 / tiles_per_wg, 262144.0 / ((t1 - t0) * 1e-3 / tiles_per_wg) / 1e9, 262144.0 * grid / ((t1 - t0) * 1e-3 / tiles_per_wg) / 1e12);
    }
    CK(hipFree(A)); CK(hipFree(W)); CK(hipFree(C));
  }
  if (mode == "ab" || mode == "all") {
    Awt L;
    if (L.open()) {
      const Problem shapes[] = {{"qkv", M, 2304, 768}, {"out", M, 768, 768}, {"fc1", M, 3072, 768}, {"fc2", M, 768, 3072}};
      for (const auto& p : shapes) ab(L, p, 5);
    }
  }
  return 0;
}
