// The dropout mask rule of the dense layers: a counter-based generator (Philox4x32-10), so the backward
// recomputes the mask of the forward instead of reading a stored one, and a row's mask does not depend
// on where in a batch the row sits (row_offset).
//
// Element (row, col) of a matrix, with a 64-bit seed, a 32-bit salt (the layer) and a probability p:
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (r & 0xffffffff, r >> 32, col >> 2, salt),  r = row + row_offset
//   word col & 3 of the output decides: keep iff word >= thr, thr = min(2^32 - 1, round(p * 2^32))
//   kept elements are multiplied by scale = 1 / (1 - p) (float32 of 1 - p, then a float32 division, as
//   torch does); dropped elements are +0.0
// One call serves four consecutive columns: what a lane holds for one 16-byte store.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace itts {

struct uint4x {
  uint32_t w[4];
};

__host__ __device__ __forceinline__ uint4x philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                         uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
#if defined(__HIP_DEVICE_COMPILE__)
    // high and low word as two 32-bit products: the 64-bit multiply-add wants aligned register pairs
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
#else
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0, h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
#endif
    const uint32_t n0 = h1 ^ c1 ^ k0;
    const uint32_t n2 = h0 ^ c3 ^ k1;
    c1 = l1;
    c3 = l0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return uint4x{{c0, c1, c2, c3}};
}

// The rule with its constants worked out on the host; passed to a kernel by value.
struct DropRule {
  static constexpr bool on = true;
  uint32_t k0, k1, salt, thr;
  float scale;   // 1 / (1 - p)
  float keep;    // 1 - p: an output d = y * scale gives y back as d * keep
  int64_t row_offset;

  // words of the four columns 4 * (col >> 2) .. + 3 of `row`
  __host__ __device__ __forceinline__ uint4x words(int64_t row, int col) const {
    const uint64_t r = (uint64_t)(row + row_offset);
    uint32_t ka = k0, kb = k1;
#if defined(__HIP_DEVICE_COMPILE__)
    // The ten round keys are uniform and the same for every call of a kernel: left alone, the compiler keeps all
    // twenty in scalar registers across a GEMM's whole K loop, which the ring kernel does not have (its spills to
    // vector registers took the epilogue beyond a wave's 128).  Opaque here, they are ten scalar additions per call.
    asm volatile("" : "+s"(ka), "+s"(kb));
#endif
    return philox4x32_10((uint32_t)r, (uint32_t)(r >> 32), (uint32_t)col >> 2, salt, ka, kb);
  }
  __host__ __device__ __forceinline__ bool keeps(uint32_t word) const { return word >= thr; }
  // bit e: column 4 * (col >> 2) + e of `row` is kept.  An epilogue works these out for all its elements first and
  // carries them in one register, so that the generator's temporaries and the activation's never live together.
  __host__ __device__ __forceinline__ uint32_t keep_bits(int64_t row, int col) const {
    const uint4x w = words(row, col);
    return (w.w[0] >= thr ? 1u : 0u) | (w.w[1] >= thr ? 2u : 0u) | (w.w[2] >= thr ? 4u : 0u) | (w.w[3] >= thr ? 8u : 0u);
  }
  __host__ __device__ __forceinline__ float apply_bit(float v, uint32_t bit) const { return bit ? v * scale : 0.f; }
  // forward (and the backward of a plain dropout): v * m * scale
  __host__ __device__ __forceinline__ float apply(float v, uint32_t word) const { return word >= thr ? v * scale : 0.f; }
};

// Stands where a kernel without dropout takes a rule: carries nothing, compiles to nothing.
struct NoDrop {
  static constexpr bool on = false;
};

static inline uint32_t drop_threshold(double p) {
  const double t = rint(p * 4294967296.0);
  return t >= 4294967295.0 ? 0xffffffffu : (t <= 0.0 ? 0u : (uint32_t)t);
}

static inline DropRule make_drop_rule(double p, uint64_t seed, uint32_t salt, int64_t row_offset) {
  DropRule d{};
  d.k0 = (uint32_t)seed;
  d.k1 = (uint32_t)(seed >> 32);
  d.salt = salt;
  d.thr = drop_threshold(p);
  d.keep = (float)(1.0 - p);
  d.scale = 1.0f / d.keep;
  d.row_offset = row_offset;
  return d;
}

// what every _dropout entry point asks of its rule
#define ITTS_REQUIRE_DROP_P(p) ITTS_REQUIRE((p) >= 0.0 && (p) < 1.0, "dropout p must be in [0, 1)")

}  // namespace itts
