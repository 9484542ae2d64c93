// Four adjacent columns of an fp32 row per lane: the access of the row-wise kernels (layernorm.hip, latent.hip,
// xent.hip, fixed_attention.hip).  With VEC -- every row 16-byte aligned, see rows16 -- a lane whose four columns all
// lie inside the row moves them as one float4; the lane that straddles the row's end, and every lane without VEC,
// moves them one by one.  Nothing at or beyond column D is written, and only load4z_pitch reads there (pad floats of
// the pitch, dropped).  The same columns land in the same lane either way.
#pragma once
#include "common.h"

namespace itts {

// rows of pitch ld starting at p may be moved as float4
static inline bool rows16(const float* p, int64_t ld) { return ld % 4 == 0 && aligned16(p); }

// columns col .. col + 3 of a row into v; the entries at or beyond column D stay as the caller set them
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ row, int col, int D, float* v) {
  if (col >= D) return;
  if (VEC && col + 3 < D) {
    const float4 t = *reinterpret_cast<const float4*>(row + col);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (col + k < D) v[k] = row[col + k];
  }
}

// .. with zeros from column D on
template <bool VEC>
__device__ __forceinline__ void load4z(const float* __restrict__ row, int col, int D, float* v) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  load4<VEC>(row, col, D, v);
}

// load4z for rows kept in registers (layernorm.hip): with VEC the lane that straddles the row's end reads its whole
// float4 as well -- the pad floats of the pitch, which rows16 says are there -- and drops what lies beyond column D.
// One path per lane instead of two: the scalar tail costs the row-in-registers kernels up to 20 VGPRs and
// ln_bwd_kernel<8, true> one of its two waves a SIMD (the backward of 20000 x 1026 rows took 152 instead of 127 us, of
// 10000 x 2047 rows 132 instead of 96; the forward was 5-25 % faster with it, which is left for a change about speed).
// The values are the same.
template <bool VEC>
__device__ __forceinline__ void load4z_pitch(const float* __restrict__ row, int col, int D, float* v) {
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (col >= D) return;
  if (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(row + col);
    v[0] = t.x;
    if (col + 1 < D) v[1] = t.y;
    if (col + 2 < D) v[2] = t.z;
    if (col + 3 < D) v[3] = t.w;
  } else {
    load4<false>(row, col, D, v);
  }
}

// .. and the store
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ row, int col, int D, const float* v) {
  if (VEC && col + 3 < D) {
    *reinterpret_cast<float4*>(row + col) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (col + k < D) row[col + k] = v[k];
  }
}

}  // namespace itts
