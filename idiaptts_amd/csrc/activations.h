// The activations fused into the GEMM epilogues (dense layers, Conv1d groups, the LDS-DMA ring):
// the ITTS_ACT_* codes of include/idiaptts_amd.h, forward y = f(z) and derivative f'(z) through y.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/idiaptts_amd.h"

namespace itts {

// tanh in ~12 VALU ops (ocml tanhf costs ~40 and showed up as ~15 % of the fused-epilogue GEMMs):
// |z| < 0.25: odd Taylor polynomial up to z^9 (truncation < 9e-9 relative);
// else 1 - 2/(exp(2|z|)+1) with the hardware exp2/rcp (abs. error <= ~1.5e-7, i.e. ~2 ulp of
// the result in [0.24, 1]).  Max deviation from torch.tanh (fp32) observed: 2.4e-7.
__device__ __forceinline__ float fast_tanhf(float z) {
  const float a = fabsf(z);
  const float z2 = z * z;
  const float poly = z * (1.f + z2 * (-0.33333334f + z2 * (0.13333334f + z2 * (-0.053968254f +
                                                                              z2 * 0.021869488f))));
  const float e = __expf(2.f * a);
  const float big = copysignf(1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f), z);
  return a < 0.25f ? poly : big;
}

// torch.nn.SELU's constants
constexpr float SELU_ALPHA = 1.6732632423543772848170429916717f;
constexpr float SELU_SCALE = 1.0507009873554804934193349852946f;

// y = f(z) with torch's default arguments (table in include/idiaptts_amd.h); accurate exp / expm1 / log1p, no
// __expf.  The clamps compare rather than fminf / fmaxf so that a NaN passes through, as in torch.
template <int ACT>
__device__ __forceinline__ float act1(float z) {
  if (ACT == ITTS_ACT_TANH) return fast_tanhf(z);
  if (ACT == ITTS_ACT_RELU) return z > 0.f ? z : 0.f;
  if (ACT == ITTS_ACT_SIGMOID) return 1.f / (1.f + expf(-z));
  if (ACT == ITTS_ACT_LOGSIGMOID) return fminf(z, 0.f) - log1pf(expf(-fabsf(z)));
  if (ACT == ITTS_ACT_SOFTPLUS) return z > 20.f ? z : log1pf(expf(z));
  if (ACT == ITTS_ACT_SOFTSIGN) return z / (1.f + fabsf(z));
  if (ACT == ITTS_ACT_LEAKY_RELU) return z > 0.f ? z : 0.01f * z;
  if (ACT == ITTS_ACT_ELU || ACT == ITTS_ACT_CELU) return z > 0.f ? z : expm1f(z);
  if (ACT == ITTS_ACT_SELU) return z > 0.f ? SELU_SCALE * z : (SELU_SCALE * SELU_ALPHA) * expm1f(z);
  if (ACT == ITTS_ACT_HARDTANH) return z < -1.f ? -1.f : (z > 1.f ? 1.f : z);
  if (ACT == ITTS_ACT_RELU6) return z < 0.f ? 0.f : (z > 6.f ? 6.f : z);
  if (ACT == ITTS_ACT_HARDSIGMOID) {
    const float t = z + 3.f;
    return (t < 0.f ? 0.f : (t > 6.f ? 6.f : t)) / 6.f;
  }
  return z;
}
// f'(z) through y = f(z); at a branch point torch's value (LeakyReLU 0.01 and ELU 1 at z = 0, the clamps 0)
template <int ACT>
__device__ __forceinline__ float dact1(float y) {
  if (ACT == ITTS_ACT_TANH) return 1.f - y * y;
  if (ACT == ITTS_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  if (ACT == ITTS_ACT_SIGMOID) return y * (1.f - y);
  if (ACT == ITTS_ACT_LOGSIGMOID) return -expm1f(y);
  if (ACT == ITTS_ACT_SOFTPLUS) return y > 20.f ? 1.f : -expm1f(-y);
  if (ACT == ITTS_ACT_SOFTSIGN) {
    const float t = 1.f - fabsf(y);
    return t * t;
  }
  if (ACT == ITTS_ACT_LEAKY_RELU) return y > 0.f ? 1.f : 0.01f;
  if (ACT == ITTS_ACT_ELU || ACT == ITTS_ACT_CELU) return y > 0.f ? 1.f : y + 1.f;
  if (ACT == ITTS_ACT_SELU) return y > 0.f ? SELU_SCALE : y + SELU_SCALE * SELU_ALPHA;
  if (ACT == ITTS_ACT_HARDTANH) return y > -1.f && y < 1.f ? 1.f : 0.f;
  if (ACT == ITTS_ACT_RELU6) return y > 0.f && y < 6.f ? 1.f : 0.f;
  if (ACT == ITTS_ACT_HARDSIGMOID) return y > 0.f && y < 1.f ? 1.f / 6.f : 0.f;
  return 1.f;
}

// run-time code -> compiled activation, for the codes of the AF_EXT family (ELU and CELU share one body);
// f(std::integral_constant<int, ACT>()) is called once
template <typename F>
__device__ __forceinline__ void with_ext_act(int act, F&& f) {
  switch (act) {
    case ITTS_ACT_SIGMOID: f(std::integral_constant<int, ITTS_ACT_SIGMOID>()); break;
    case ITTS_ACT_LOGSIGMOID: f(std::integral_constant<int, ITTS_ACT_LOGSIGMOID>()); break;
    case ITTS_ACT_SOFTPLUS: f(std::integral_constant<int, ITTS_ACT_SOFTPLUS>()); break;
    case ITTS_ACT_SOFTSIGN: f(std::integral_constant<int, ITTS_ACT_SOFTSIGN>()); break;
    case ITTS_ACT_LEAKY_RELU: f(std::integral_constant<int, ITTS_ACT_LEAKY_RELU>()); break;
    case ITTS_ACT_ELU:
    case ITTS_ACT_CELU: f(std::integral_constant<int, ITTS_ACT_ELU>()); break;
    case ITTS_ACT_SELU: f(std::integral_constant<int, ITTS_ACT_SELU>()); break;
    case ITTS_ACT_HARDTANH: f(std::integral_constant<int, ITTS_ACT_HARDTANH>()); break;
    case ITTS_ACT_RELU6: f(std::integral_constant<int, ITTS_ACT_RELU6>()); break;
    default: f(std::integral_constant<int, ITTS_ACT_HARDSIGMOID>()); break;
  }
}

// Activation family of a kernel instantiation: AF_BASE picks NONE / TANH / RELU at run time (the headline FF step's
// kernels, whose code the other activations must leave alone); AF_EXT picks among codes 3 .. 13.  The host
// chooses the family from the code.
enum { AF_BASE = 0, AF_EXT = 1 };
static inline int act_family(int act) { return act >= ITTS_ACT_SIGMOID ? AF_EXT : AF_BASE; }

// the AF_BASE family, code chosen at run time
__device__ __forceinline__ float act_fwd(float z, int act) {
  if (act == ITTS_ACT_TANH) return fast_tanhf(z);
  if (act == ITTS_ACT_RELU) return z > 0.f ? z : 0.f;
  return z;
}
__device__ __forceinline__ float act_grad_from_out(float y, int act) {
  if (act == ITTS_ACT_TANH) return 1.f - y * y;
  if (act == ITTS_ACT_RELU) return y > 0.f ? 1.f : 0.f;
  return 1.f;
}

// either family: a run-time code of the family AF
template <int AF>
__device__ __forceinline__ float act_fwd_af(float z, int act) {
  if (AF == AF_BASE) return act_fwd(z, act);
  float y = z;
  with_ext_act(act, [&](auto a) { y = act1<decltype(a)::value>(z); });
  return y;
}
template <int AF>
__device__ __forceinline__ float act_grad_af(float y, int act) {
  if (AF == AF_BASE) return act_grad_from_out(y, act);
  float d = 1.f;
  with_ext_act(act, [&](auto a) { d = dact1<decltype(a)::value>(y); });
  return d;
}

}  // namespace itts
