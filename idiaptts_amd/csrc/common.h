// Shared host/device helpers for the gfx950 kernels of libidiaptts_amd.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/idiaptts_amd.h"

namespace itts {

void set_error(const std::string& msg);

#define ITTS_HIP_CHECK(expr)                                                              \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) {                                                               \
      ::itts::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));               \
      return ITTS_E_HIP;                                                                  \
    }                                                                                     \
  } while (0)

// (`entry`: the entry point that the message names; a body that serves several of them says which one was called)
#define ITTS_REQUIRE_AS(entry, cond, msg)                                                 \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      ::itts::set_error(std::string(entry) + ": " + (msg));                               \
      return ITTS_E_INVALID;                                                              \
    }                                                                                     \
  } while (0)

#define ITTS_REQUIRE(cond, msg) ITTS_REQUIRE_AS(__func__, cond, msg)

#define ITTS_LAUNCH_CHECK() ITTS_HIP_CHECK(hipGetLastError())

// Host wait for everything queued on `s`, by polling: hipStreamSynchronize puts the thread to
// sleep when the wait gets long (a millisecond-scale kernel in front) and the wake-up then costs
// up to a millisecond of idle GPU; data-dependent loops that need a count back from the device
// between launches (mcep trip counts) poll an event instead.
static inline hipError_t itts_spin_sync(hipStream_t s) {
  hipEvent_t ev;
  hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) return e;
  e = hipEventRecord(ev, s);
  if (e == hipSuccess)
    while ((e = hipEventQuery(ev)) == hipErrorNotReady) {
    }
  (void)hipEventDestroy(ev);
  return e;
}

constexpr int kWave = 64;  // gfx950 wavefront

// one step of a butterfly sum: v plus the value of the lane whose number differs in the bits of mask
__device__ __forceinline__ double xor_sum(double v, int mask) { return v + __shfl_xor(v, mask, 64); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Block-wide sum for blockDim.x a multiple of 64 (<= 1024). `red` needs 16 doubles of LDS.
// Result valid in every thread.
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < nw; ++i) s += red[i];  // same order in every thread: deterministic
  return s;
}

// Scratch memory of the entry points.  hipMallocAsync's pool hands its blocks back to the driver
// whenever a request does not fit what it has cached (one Harvest call empties it), and a fresh
// device allocation occasionally takes hundreds of milliseconds to seconds on this platform
// (measured: an analysis pass of 65 ms took 2.3 s right after the pool had been emptied; a whole
// bench process ran its analysis section at 330 ms per pass).  So the library keeps its own
// blocks (context.hip): a request gets a cached block of its size class (plain hipMalloc the first
// time), a release marks the block free behind an event on the releasing stream, and a block that
// moves to another stream waits for that event first (stream-ordered like hipMallocAsync /
// hipFreeAsync).  At most ITTS_POOL_KEEP_GB (default 64) stay cached; itts_release_scratch() frees
// everything that is not in use.
//
// A ScratchScope is the only way to the pool, and it owns what is taken through it: take() hands out
// `count` elements of T, and the destructor releases every block the scope took, behind the work
// already queued on its stream -- at the end of the entry point and at every early return of
// ITTS_REQUIRE / ITTS_HIP_CHECK / ITTS_LAUNCH_CHECK alike.  There is no separate free.  Blocks that
// must go back before a later request of the same call (so that the request can reuse them) live in
// a nested scope in a C++ block of their own.  A helper that allocates for its caller takes the
// caller's ScratchScope&.
class ScratchScope {
 public:
  explicit ScratchScope(hipStream_t s) : stream_(s) {}
  ~ScratchScope();
  ScratchScope(const ScratchScope&) = delete;
  ScratchScope& operator=(const ScratchScope&) = delete;

  template <typename T>
  hipError_t take(T** out, size_t count) {
    return take_bytes(reinterpret_cast<void**>(out), count * sizeof(T));
  }
  hipStream_t stream() const { return stream_; }

 private:
  hipError_t take_bytes(void** out, size_t bytes);
  hipStream_t stream_;
  std::vector<void*> blocks_;
};

// Raises the dynamic-LDS limit of `kernel` on the current device to at least `bytes` (launches above
// 64 KB need it).  Grow-only and thread-safe; the runtime is asked only when this (device, kernel)
// pair has not been granted that much yet.
hipError_t allow_dynamic_lds(const void* kernel, size_t bytes);

// Sum of S split-K slabs of n floats (slab s at slabs + s * n) into out (nn.hip): the reduction of
// itts_linear_bwd_weight, queued instead of launched inside itts_defer_reductions.
int reduce_slabs(const float* slabs, int S, int64_t n, float* out, int accumulate, hipStream_t s);

// *loss = (float)(scale * sum of the nb partial sums), one launch of one workgroup in a fixed order (nn.hip): the
// last step of every loss entry point.
int loss_final_sum(const double* partial, int64_t nb, double scale, float* loss, hipStream_t s);

// y = act(x w^T + b) of a dense layer (nn.hip): the body of itts_linear_fwd (DR = NoDrop) and itts_linear_fwd_dropout
// (DR = DropRule, dropout.h), here for the sparse-input entry point's way to the dense product.
template <class DR>
int linear_fwd(const float* d_x, int64_t ldx, const float* d_w, const float* d_b, float* d_y, int64_t ldy, int64_t M,
               int N, int K, int act, hipStream_t s, const DR& dr);

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// 16-byte aligned: with a pitch that is a multiple of 4 floats, rows may be read as float4
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace itts
