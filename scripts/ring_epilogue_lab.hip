// Lab: what the epilogue of the ring GEMM (csrc/gemm_ring.h) costs at the short-reduction shapes of the
// FF train step, split by the header's RING_DBG switches.  One program per switch value:
//
//   for d in 0 8 32 64; do
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=on -I idiaptts_amd/csrc -DRING_DBG=$d \
//           scripts/ring_epilogue_lab.hip -o build/ring_epilogue_lab_$d
//   done
//
//   RING_DBG=0   the product kernels
//   RING_DBG=8   no epilogue at all               -> (0) - (8)   = the whole epilogue
//   RING_DBG=32  early operands are constants     -> (0) - (32)  = what their global loads still cost
//   RING_DBG=64  no stores                        -> (0) - (64)  = what the stores cost
//
// Each shape runs 300 launches unmeasured (the clock follows the previous kernel for milliseconds), then
// 400 between two events; prints the mean microseconds per launch and, from the per-workgroup stamps
// of one more launch, the longest and the mean workgroup lifetime in 100 MHz ticks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemm_ring.h"

using namespace itts;

#define CK(x)                                                                                   \
  do {                                                                                          \
    hipError_t e_ = (x);                                                                        \
    if (e_ != hipSuccess) {                                                                     \
      std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_));            \
      std::exit(1);                                                                             \
    }                                                                                           \
  } while (0)

static float* dev_floats(size_t n, float lo, float hi) {
  std::vector<float> h(n);
  uint32_t s = 12345u + (uint32_t)n;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    h[i] = lo + (hi - lo) * (float)(s >> 8) * (1.0f / 16777216.0f);
  }
  float* d;
  CK(hipMalloc(&d, n * 4));
  CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
  return d;
}

template <bool A_ROW, bool B_ROW, int EPI>
static void run(const char* name, int M, int N, int K, int ldaux) {
  constexpr int BMT = 128, BNT = 64;
  const int lda = A_ROW ? (K + 3) / 4 * 4 : 0, ldb = B_ROW ? (K + 3) / 4 * 4 : (N + 3) / 4 * 4, ldc = (N + 3) / 4 * 4;
  ring::Args r{};
  r.A = dev_floats((size_t)M * lda, -1.f, 1.f);
  r.B = dev_floats(B_ROW ? (size_t)N * ldb : (size_t)K * ldb, -0.05f, 0.05f);
  r.C = dev_floats((size_t)M * ldc, 0.f, 0.f);
  r.aux = dev_floats((size_t)M * ldaux, -0.9f, 0.9f);
  r.bias = EPI != ring::EPI_DACT ? dev_floats(N, -0.5f, 0.5f) : nullptr;
  uint8_t* rv;
  CK(hipMalloc(&rv, M));
  CK(hipMemset(rv, 1, M));
  r.row_valid = rv;
  double* lp;
  CK(hipMalloc(&lp, 512 * 8));
  r.loss_partial = lp;
  r.lda = lda; r.ldb = ldb; r.ldc = ldc; r.ldaux = ldaux;
  r.M = M; r.N = N; r.K = K; r.kchunk = (K + 31) / 32 * 32; r.splitk = 1;
  r.tiles_m = (M + BMT - 1) / BMT; r.tiles_n = (N + BNT - 1) / BNT; r.gn = r.tiles_n;
  r.act = ITTS_ACT_TANH; r.gscale = 1e-3f;
  const int ntiles = r.tiles_m * r.tiles_n;
  const int grid = std::min(512, (ntiles + 7) / 8 * 8);
  auto launch = [&]() {
    hipLaunchKernelGGL((ring::gemm_ring_kernel<A_ROW, B_ROW, EPI, 2>), dim3(grid), dim3(ring::THREADS), 0, 0, r);
  };
  for (int i = 0; i < 300; ++i) launch();
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipEventRecord(e0, 0));
  for (int i = 0; i < 400; ++i) launch();
  CK(hipEventRecord(e1, 0));
  CK(hipEventSynchronize(e1));
  float ms = 0.f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  uint64_t* st;
  CK(hipMalloc(&st, (size_t)grid * 4 * 8));
  CK(hipMemset(st, 0, (size_t)grid * 4 * 8));
  r.stamps = st;
  launch();
  CK(hipDeviceSynchronize());
  std::vector<uint64_t> hs((size_t)grid * 4);
  CK(hipMemcpy(hs.data(), st, hs.size() * 8, hipMemcpyDeviceToHost));
  double mean = 0.0;
  uint64_t longest = 0;
  for (int b = 0; b < grid; ++b) {
    mean += (double)hs[4 * b + 1] / grid;
    longest = std::max(longest, hs[4 * b + 1]);
  }
  std::printf("RING_DBG=%d %-22s M=%d N=%d K=%d tiles=%d  %.2f us/launch  workgroup ticks(100MHz): mean %.0f longest %llu\n",
              RING_DBG, name, M, N, K, ntiles, ms * 1000.f / 400.f, mean, (unsigned long long)longest);
  std::fflush(stdout);
}

int main(int argc, char** argv) {
  const int M = argc > 1 ? std::atoi(argv[1]) : 38019;
  run<true, true, ring::EPI_MSE>("fwd3+MSE", M, 187, 512, 187);
  run<true, false, ring::EPI_DACT>("dX2 (K=187, DACT)", M, 512, 187, 512);
  run<true, false, ring::EPI_DACT>("dX1 (K=512, DACT)", M, 512, 512, 512);
  run<true, true, ring::EPI_BIAS_ACT>("fwd2 (BIAS_ACT)", M, 512, 512, 512);
  return 0;
}
