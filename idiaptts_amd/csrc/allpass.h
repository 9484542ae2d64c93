// All-pass frequency warping of cepstral rows (csrc/allpass.hip): what the C entry points in capi.hip hand to the
// launchers.  All checks of sizes and pointers are the entry points'.
#pragma once
#include "common.h"

namespace itts {

constexpr int kAllpassMaxN = 64;  // coefficients per block the kernels take (one LDS column of 64 lanes each)

struct AllpassArgs {
  const float* x; int64_t ldx;      // [M, D] input rows (never written)
  const float* alpha;               // [M] warping factor of each row
  const float* mean; const float* sd;   // [D] each, either may be null
  float* y; int64_t ldy;            // forward: [M, D] output rows
  const float* dy; int64_t lddy;    // backward: gradient of the output rows
  float* dx; int64_t lddx;          // backward: gradient of the input rows
  float* dalpha;                    // backward: [M]
  int64_t M;
  int N, nb;                        // D = nb * N
};

hipError_t allpass_launch_fwd(const AllpassArgs& a, hipStream_t s);
hipError_t allpass_launch_bwd(const AllpassArgs& a, hipStream_t s);

}  // namespace itts
