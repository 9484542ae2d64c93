// Weight gradient of the first dense layer on a sparse input for gfx950: dw = dz^T x without the products by x's
// exact zeros (sparse_rows.hip is the forward's side of the same input).  The accumulators stay in registers, so
// the non-zeros are walked by column: once per batch sparse_cols_build_kernel cuts x into tiles of 256 rows and
// writes, per tile, the (row, value) lists of the light columns and a compact strip of the heavy ones
// (sparse_cols_from_rows_kernel writes the same from the forward's row lists, without reading x); the plan
// (itts_sparse_cols_* in the header) says which column is which and who owns it.
//   * light columns: a quarter wave owns up to 8 of them and keeps a float4 accumulator per column and lane (four
//     adjacent dz columns); per list entry one DPP row broadcast, one 16-byte LDS read of the dz row, four fmaf.
//     Roofline: instruction issue, as in the forward walk.
//   * heavy columns (and the bias, as a column of ones): v_mfma_f32_32x32x2_f32 on dz_tile^T [64 x 256] times the
//     strip tile [256 x 32].
#include <algorithm>
#include <atomic>

#include "common.h"

namespace itts {

constexpr int kWgMaxK = 512;          // 64 owners x 8 columns; the transposed output tile [64][513] fits the LDS
constexpr int kTile = 256;            // rows of a tile
constexpr int kSlab = 64;             // dz columns of a workgroup
constexpr int kWgWaves = 16;          // one workgroup per CU (LDS), four waves per SIMD
constexpr int kOwners = 64;           // quarter waves of a workgroup
constexpr int kSlots = 8;             // light columns of an owner
constexpr int kStrip = 32;            // heavy strip: up to 31 columns of x and a column of ones
constexpr int kBlock = 16;            // list entries per load: one per lane of a quarter wave
constexpr int kGroup = 4;             // entries between two tests of the list's end
// The lists of a (tile, owner, slot) hold at most 256 entries, 16 blocks, and nothing is capped; but a light
// column's list rarely needs a second block, so block 0 of every list lies in one compact array (64 KB a tile:
// what the walk usually reads stays together in the caches and the TLB) and blocks 1..15 in a second, mostly
// untouched one.  The counts, 8 x uint16 per (tile, owner), lie in front of both.
constexpr int kHeaderBytes = kSlots * 2;
constexpr int kFirstBytes = kBlock * 8;
constexpr int kOverBytes = (kTile / kBlock - 1) * kBlock * 8;
// the plan: strip columns, (owner, slot) -> column, and the inverse column -> owner * 8 + slot or kHeavyCode + h
constexpr int kPlanInv = kStrip + kOwners * kSlots;
constexpr int kPlanInts = kPlanInv + kWgMaxK;
constexpr int kHeavyCode = 0x1000;
constexpr int kRowBytes = kSlab * 4;
constexpr int kBufBytes = (kTile + 1) * kRowBytes;   // a dz tile and an all-zero row for the neutral entries
constexpr int kTPitch = 513;                         // odd: the transposing writes spread over the banks
constexpr int kBiasFloat = 2 * kBufBytes / 4;        // the bias sums sit behind the two tile buffers
constexpr int kWgLdsBytes = 2 * kBufBytes + kSlab * 4;
static_assert(kSlab * kTPitch * 4 <= 2 * kBufBytes, "the output tile reuses the dz buffers");

static std::atomic<int64_t> g_wgrad_path[3];

struct ColsLayout {
  int64_t tiles, strip_off, streams_off, bytes;   // streams: headers, first blocks, further blocks
};

static ColsLayout cols_layout(int64_t M) {
  ColsLayout l;
  l.tiles = (M + kTile - 1) / kTile;
  l.strip_off = 0;
  l.streams_off = l.tiles * kTile * kStrip * 4;
  l.bytes = l.streams_off + l.tiles * kOwners * (int64_t)(kHeaderBytes + kSlots * (kFirstBytes + kOverBytes));
  return l;
}

// where the parts of the streams start, and entry j of list `pair` = (tile * 64 + owner) * 8 + slot
__device__ __forceinline__ const char* firsts_of(const char* streams, int tiles) {
  return streams + (int64_t)tiles * kOwners * kHeaderBytes;
}
__device__ __forceinline__ const char* overs_of(const char* streams, int tiles) {
  return firsts_of(streams, tiles) + (int64_t)tiles * kOwners * kSlots * kFirstBytes;
}
__device__ __forceinline__ int2* entry_of(char* streams, int tiles, int64_t pair, int j) {
  char* p = j < kBlock ? const_cast<char*>(firsts_of(streams, tiles)) + pair * kFirstBytes + j * 8
                       : const_cast<char*>(overs_of(streams, tiles)) + pair * kOverBytes + (j - kBlock) * 8;
  return reinterpret_cast<int2*>(p);
}

// Grid = (tile, parts + 1).  Part p serves columns 64 p .. 64 p + 63, a lane one column (the reads of x are
// coalesced), a wave one quarter of the tile's rows.  A lane reads its 64 values and looks its column up in the
// plan's inverse.  Light: the four waves exchange their counts through LDS, every lane then knows where its rows go
// inside the column's list (ascending rows without sorting or atomics), whose place in the owner's stream is
// fixed by the slot.  An entry is {byte offset of the dz row in the LDS tile, value}; the last block is filled up
// with neutral entries (the tile's all-zero row, +0).  Heavy: the values go to the column's place in the strip.
// The last part writes what no column writes: the strip columns without a column of x (zeros; ones in column 31)
// and the zero counts of the slots without one.
__global__ __launch_bounds__(256) void sparse_cols_build_kernel(const uint32_t* __restrict__ x, int64_t ldx, int64_t M,
                                                                int K, int parts, int tiles,
                                                                const int* __restrict__ plan,
                                                                uint32_t* __restrict__ strip,
                                                                char* __restrict__ streams) {
  __shared__ int cnts[4][64];
  const int tile = (int)(blockIdx.x / (parts + 1)), part = (int)(blockIdx.x % (parts + 1));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)tile * kTile + wave * 64;
  if (part == parts) {
    const int h = lane & 31;
    const int hc = h < kStrip - 1 ? plan[h] : -1;
    if (!(hc >= 0 && hc < K)) {
      for (int i = 0; i < 32; ++i) {
        const int64_t m = m0 + 2 * i + (lane >> 5);   // rows behind M are zeros: the strip covers whole tiles
        strip[m * kStrip + h] = (m < M && h == kStrip - 1) ? 0x3f800000u : 0u;
      }
    }
    for (int pair = threadIdx.x; pair < kOwners * kSlots; pair += 256) {
      const int c = plan[kStrip + pair];
      if (!(c >= 0 && c < K))
        reinterpret_cast<uint16_t*>(streams + ((int64_t)tile * kOwners + pair / kSlots) * kHeaderBytes)[pair % kSlots] = 0;
    }
    return;
  }
  const int k = part * 64 + lane;
  const bool valid = k < K;
  const int code = valid ? plan[kPlanInv + k] : -1;
  const bool light = code >= 0 && code < kOwners * kSlots;
  const bool heavy = code >= kHeavyCode && code < kHeavyCode + kStrip - 1;
  uint32_t bits[64];
#pragma unroll
  for (int r = 0; r < 64; ++r) bits[r] = (valid && m0 + r < M) ? x[(m0 + r) * ldx + k] : 0u;
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < 64; ++r) cnt += (bits[r] & 0x7fffffffu) != 0u ? 1 : 0;   // +-0.0 out; NaN and denormals stay
  cnts[wave][lane] = cnt;
  __syncthreads();
  if (heavy) {
    uint32_t* dst = strip + m0 * kStrip + (code - kHeavyCode);
#pragma unroll
    for (int r = 0; r < 64; ++r) dst[r * kStrip] = bits[r];
  }
  if (!light) return;
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int c = cnts[w][lane];
    before += w < wave ? c : 0;
    total += c;
  }
  const int owner = code / kSlots, slot = code % kSlots;
  const int64_t pair = ((int64_t)tile * kOwners + owner) * kSlots + slot;
  int j = before;
#pragma unroll
  for (int r = 0; r < 64; ++r)
    if ((bits[r] & 0x7fffffffu) != 0u)
      *entry_of(streams, tiles, pair, j++) = make_int2((wave * 64 + r) * kRowBytes, (int)bits[r]);
  if (wave == 0) {
    const int end = (total + kBlock - 1) / kBlock * kBlock;
    for (int e = total; e < end; ++e) *entry_of(streams, tiles, pair, e) = make_int2(kTile * kRowBytes, 0);
    reinterpret_cast<uint16_t*>(streams + ((int64_t)tile * kOwners + owner) * kHeaderBytes)[slot] = (uint16_t)total;
  }
}

// The same column block from the row lists of x (sparse_rows.hip) instead of x itself: the lists already name every
// non-zero, so nothing dense is read or compacted.  Workgroup = tile of 256 rows, wave = 16 consecutive rows, half
// wave = row, lane = two adjacent list entries (one 16-byte load); block 0 of the tile's 512 lists and its strip
// tile are put together in LDS and leave as whole lines.
//   fill:   mask words and strip zeros (column 31: ones in front of M), every list of `first` neutral entries, the
//           plan's inverse; meanwhile the first 64 slots of the wave's 16 rows and their counts are on their way
//           into registers (together: what lies behind a row's count is read and masked out)
//   mark:   word[wave][list of the entry's column] |= 1 << row of the wave (an integer OR in LDS: no order changes
//           the word); entries of columns >= K are nobody's
//   prefix: lane = list: the upper half of each of the list's 16 words becomes the number of entries in the waves
//           before it, the total the header
//   place:  position = entries before the wave + marked rows of the wave before this one: ascending rows inside
//           every list, without a counter.  A position < 16 lands in `first`, a later one goes straight to its
//           overflow block (8-byte stores, as the build from x); a heavy column's value lands in the strip tile
//   out:    64 KB of first blocks and 32 KB of strip, 16 bytes a lane; then the neutral tails of the lists that
//           end beyond block 0
// A row of more than 64 entries takes further trips, read again in both sweeps.
constexpr int kFromRowsWaves = 16;
constexpr int kFromRowsPairs = kTile / kFromRowsWaves / 2;   // row pairs of a wave
constexpr int kLists = kOwners * kSlots;
constexpr int kFromRowsLdsBytes = kLists * kFirstBytes + kTile * kStrip * 4 + kFromRowsWaves * kLists * 4 + kWgMaxK * 4;

__global__ __launch_bounds__(kFromRowsWaves * 64) void sparse_cols_from_rows_kernel(
    const int* __restrict__ counts, const int4* __restrict__ entries2, int64_t pitch2, int64_t M, int K, int tiles,
    const int* __restrict__ plan, uint32_t* __restrict__ strip, char* __restrict__ streams) {
  constexpr int T = kFromRowsWaves * 64;
  extern __shared__ uint4 from_rows_lds[];
  int2* first = reinterpret_cast<int2*>(from_rows_lds);                          // [512 lists][16]
  uint32_t* tile_strip = reinterpret_cast<uint32_t*>(first + kLists * kBlock);   // [256][32]
  uint32_t* words = tile_strip + kTile * kStrip;                                 // [16 waves][512 lists]
  int* inverse = reinterpret_cast<int*>(words + kFromRowsWaves * kLists);        // [512 columns]
  const int tid = threadIdx.x, lane = tid & 63, l32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = (int)blockIdx.x;
  const int64_t m0 = (int64_t)tile * kTile;
  const int row0 = wave * 2 * kFromRowsPairs + (lane >> 5);   // this lane's row of pair q: row0 + 2 q

  int code_of_tid = -1;   // light: the list; heavy: as in the plan; else nobody's
  if (tid < K) {
    const int code = plan[kPlanInv + tid];
    if ((code >= 0 && code < kLists) || (code >= kHeavyCode && code < kHeavyCode + kStrip - 1)) code_of_tid = code;
  }
  int cnt[kFromRowsPairs];
  int4 head[kFromRowsPairs];   // {column, value} of entries 2 l32 and 2 l32 + 1, later {code, value}
#pragma unroll
  for (int q = 0; q < kFromRowsPairs; ++q) {
    const int64_t m = m0 + row0 + 2 * q;
    const bool in = m < M && l32 < pitch2;
    cnt[q] = in ? std::min(counts[m], (int)(2 * pitch2)) : 0;
    head[q] = in ? entries2[m * pitch2 + l32] : make_int4(-1, 0, -1, 0);
  }

  {
    const uint4 neutral = make_uint4((uint32_t)(kTile * kRowBytes), 0u, (uint32_t)(kTile * kRowBytes), 0u);
    uint4* first4 = reinterpret_cast<uint4*>(first);
    for (int i = tid; i < kLists * kFirstBytes / 16; i += T) first4[i] = neutral;
    uint4* strip4 = reinterpret_cast<uint4*>(tile_strip);
    for (int i = tid; i < kTile * kStrip / 4; i += T) {
      const bool ones = (i & 7) == 7 && m0 + (i >> 3) < M;   // the last four columns of row i / 8
      strip4[i] = make_uint4(0u, 0u, 0u, ones ? 0x3f800000u : 0u);
    }
    uint4* words4 = reinterpret_cast<uint4*>(words);
    for (int i = tid; i < kFromRowsWaves * kLists / 4; i += T) words4[i] = make_uint4(0u, 0u, 0u, 0u);
    if (tid < kWgMaxK) inverse[tid] = code_of_tid;
  }
  int most = 0;
#pragma unroll
  for (int q = 0; q < kFromRowsPairs; ++q) {
    if (2 * l32 >= cnt[q]) head[q].x = -1;
    if (2 * l32 + 1 >= cnt[q]) head[q].z = -1;
    most = std::max(most, cnt[q]);
  }
  const bool further = std::max(most, __shfl_xor(most, 32, 64)) > 64;   // uniform in the wave
  __syncthreads();

  uint32_t* my_words = words + wave * kLists;
  auto code_of = [&](int k) { return (unsigned)k < (unsigned)K ? inverse[k] : -1; };
  auto again = [&](int q, int j0) {   // entries j0 + 2 l32 and the next of the lane's row
    int4 e = j0 + 2 * l32 < cnt[q] ? entries2[(m0 + row0 + 2 * q) * pitch2 + j0 / 2 + l32] : make_int4(-1, 0, -1, 0);
    if (j0 + 2 * l32 + 1 >= cnt[q]) e.z = -1;
    e.x = code_of(e.x);
    e.z = code_of(e.z);
    return e;
  };
  auto mark = [&](int q, int code) {
    if (code >= 0 && code < kLists) atomicOr(&my_words[code], 1u << (2 * q + (lane >> 5)));
  };
  auto place = [&](int q, int code, int value) {
    const int row = 2 * q + (lane >> 5);   // of the wave
    if (code >= 0 && code < kLists) {
      const uint32_t word = my_words[code];
      const int pos = (int)(word >> 16) + __popc(word & ((1u << row) - 1u));
      const int2 out = make_int2((row0 + 2 * q) * kRowBytes, value);
      if (pos < kBlock) first[code * kBlock + pos] = out;
      else if (pos < kTile) *entry_of(streams, tiles, (int64_t)tile * kLists + code, pos) = out;
    } else if (code >= kHeavyCode) {
      tile_strip[(row0 + 2 * q) * kStrip + (code - kHeavyCode)] = (uint32_t)value;
    }
  };

#pragma unroll
  for (int q = 0; q < kFromRowsPairs; ++q) {
    head[q].x = code_of(head[q].x);
    head[q].z = code_of(head[q].z);
  }
#pragma unroll
  for (int q = 0; q < kFromRowsPairs; ++q) {
    mark(q, head[q].x);
    mark(q, head[q].z);
  }
  if (further) {
#pragma unroll
    for (int q = 0; q < kFromRowsPairs; ++q)
      for (int j0 = 64; j0 < cnt[q]; j0 += 64) {
        const int4 e = again(q, j0);
        mark(q, e.x);
        mark(q, e.z);
      }
  }
  __syncthreads();

  if (tid < kLists) {
    int run = 0;
#pragma unroll
    for (int w = 0; w < kFromRowsWaves; ++w) {
      const uint32_t rows_of_wave = words[w * kLists + tid];
      words[w * kLists + tid] = rows_of_wave | ((uint32_t)run << 16);
      run += __popc(rows_of_wave);
    }
    reinterpret_cast<uint16_t*>(streams)[(int64_t)tile * kLists + tid] = (uint16_t)run;
  }
  __syncthreads();

#pragma unroll
  for (int q = 0; q < kFromRowsPairs; ++q) {
    place(q, head[q].x, head[q].y);
    place(q, head[q].z, head[q].w);
  }
  if (further) {
#pragma unroll
    for (int q = 0; q < kFromRowsPairs; ++q)
      for (int j0 = 64; j0 < cnt[q]; j0 += 64) {
        const int4 e = again(q, j0);
        place(q, e.x, e.y);
        place(q, e.z, e.w);
      }
  }
  __syncthreads();

  {
    const uint4* first4 = reinterpret_cast<const uint4*>(first);
    uint4* dst = reinterpret_cast<uint4*>(const_cast<char*>(firsts_of(streams, tiles)) +
                                          (int64_t)tile * kLists * kFirstBytes);
    for (int i = tid; i < kLists * kFirstBytes / 16; i += T) dst[i] = first4[i];
    const uint4* strip4 = reinterpret_cast<const uint4*>(tile_strip);
    uint4* sdst = reinterpret_cast<uint4*>(strip + m0 * kStrip);
    for (int i = tid; i < kTile * kStrip / 4; i += T) sdst[i] = strip4[i];
  }
  {   // two threads a list: the neutral entries behind its last one, up to a whole block
    const int list = tid & (kLists - 1);
    const uint32_t last = words[(kFromRowsWaves - 1) * kLists + list];
    const int total = (int)(last >> 16) + __popc(last & 0xffffu);
    if (total > kBlock) {
      const int end = (total + kBlock - 1) / kBlock * kBlock;
      for (int e = total + (tid >> 9); e < end; e += T / kLists)
        *entry_of(streams, tiles, (int64_t)tile * kLists + list, e) = make_int2(kTile * kRowBytes, 0);
    }
  }
}

typedef float floatx16 __attribute__((ext_vector_type(16)));

// Entry J of the 16 a quarter wave holds, one per lane: the DPP row broadcast hands lane J's (row offset, value) to
// the quarter's 16 lanes, which read their 16 bytes of that dz row and do four fmaf.
template <int J>
__device__ __forceinline__ void col_slot(const char* buf, int lane_off, int2 e, float4& acc) {
  // (row_newbcast writes every lane: with bound_ctrl nothing zeroes the destinations first)
  const int off = __builtin_amdgcn_update_dpp(0, e.x, 0x150 + J, 0xf, 0xf, true);   // row_newbcast:J
  const float v = __int_as_float(__builtin_amdgcn_update_dpp(0, e.y, 0x150 + J, 0xf, 0xf, true));
  const float4 d = *reinterpret_cast<const float4*>(buf + off + lane_off);
  acc.x = fmaf(v, d.x, acc.x); acc.y = fmaf(v, d.y, acc.y);
  acc.z = fmaf(v, d.z, acc.z); acc.w = fmaf(v, d.w, acc.w);
}
template <int FIRST>
__device__ __forceinline__ void col_group(const char* buf, int lane_off, int2 e, float4& acc) {
  col_slot<FIRST>(buf, lane_off, e, acc);
  col_slot<FIRST + 1>(buf, lane_off, e, acc);
  col_slot<FIRST + 2>(buf, lane_off, e, acc);
  col_slot<FIRST + 3>(buf, lane_off, e, acc);
}

// Workgroup = (64-column slab of dz, range of row tiles).  The dz tiles [256][64] alternate between two LDS buffers:
// the next tile's 16-byte loads go out behind the walk of the current one and are stored behind its MFMAs, one
// barrier per tile; dz is read from memory once.
//   light: quarter wave `owner` reads its lists of the tile in blocks of 16 entries, block 0 of all eight fetched
//     a tile ahead, further blocks a list or two blocks ahead; for each of its 8 columns (statically unrolled: the
//     accumulators are registers) the wave runs to the longest of its four quarters' lists in groups of 4 entries,
//     a quarter whose list has ended sits them out.
//   heavy: waves 0..7 take dz columns 0..31, waves 8..15 columns 32..63, each 32 rows of the tile: 16 MFMAs
//     32x32x2 with A = dz^T from LDS (lane = column: conflict free) and B = the strip rows straight from memory.
// Order of the sums: a light column's fmaf chain runs over the range's rows in ascending m from +0; a heavy
// column's (and the bias's) over the rows of a wave's share, tile after tile, then the shares in wave order (parked
// in LDS by every wave at once and summed by one thread per cell: one barrier, not a round per wave); the ranges are
// the slabs of the usual split-K workspace and are added in slab order by the usual reduction.
__global__ __launch_bounds__(kWgWaves * 64) void sparse_wgrad_kernel(
    const float* __restrict__ dz, int64_t lddz, const float* __restrict__ strip, const char* __restrict__ streams,
    const int* __restrict__ plan, float* __restrict__ slabs, int64_t slab_stride, int lddw,
    float* __restrict__ bias_part, int64_t bias_stride, int64_t M, int N, int K, int tiles, int per, int ranges) {
  extern __shared__ float4 smem4[];
  char* smem = reinterpret_cast<char*>(smem4);
  float* smemf = reinterpret_cast<float*>(smem4);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, owner = wave * 4 + (lane >> 4);
  const int n0 = (int)(blockIdx.x / ranges) * kSlab;
  const int range = (int)(blockIdx.x % ranges);
  const int t_begin = range * per, t_end = std::min(tiles, t_begin + per);

  if (tid < 128) smemf[((tid >> 6) * kBufBytes + kTile * kRowBytes) / 4 + lane] = 0.f;   // the all-zero rows

  const int srow = tid >> 4, c4 = (tid & 15) * 4, n = n0 + c4;
  auto load_tile = [&](int t, float4 (&st)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int64_t m = (int64_t)t * kTile + p * 64 + srow;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < M) {
        const float* src = dz + m * lddz + n;
        if (n + 4 <= N) {
          v = *reinterpret_cast<const float4*>(src);
        } else {
          if (n < N) v.x = src[0];
          if (n + 1 < N) v.y = src[1];
          if (n + 2 < N) v.z = src[2];
        }
      }
      st[p] = v;
    }
  };
  auto store_tile = [&](int b, const float4 (&st)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
      *reinterpret_cast<float4*>(smem + b * kBufBytes + (p * 64 + srow) * kRowBytes + c4 * 4) = st[p];
  };
  const char* firsts = firsts_of(streams, tiles) + i16 * 8;
  const char* overs = overs_of(streams, tiles) + i16 * 8;
  auto lists_of = [&](int t) { return ((int64_t)t * kOwners + owner) * kSlots; };

  float4 acc[kSlots];
#pragma unroll
  for (int c = 0; c < kSlots; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
  floatx16 hacc;
#pragma unroll
  for (int r = 0; r < 16; ++r) hacc[r] = 0.f;

  // what a tile's walk starts from: the counts and block 0 of each of the 8 lists.  All nine loads go out
  // together, a tile ahead (their places do not depend on the counts), so a walk waits for memory once and not
  // once per list.
  uint4 hdr;
  int2 first[kSlots];
  auto load_lists = [&](int t) {
    hdr = *reinterpret_cast<const uint4*>(streams + ((int64_t)t * kOwners + owner) * kHeaderBytes);
#pragma unroll
    for (int c = 0; c < kSlots; ++c)
      first[c] = *reinterpret_cast<const int2*>(firsts + (lists_of(t) + c) * kFirstBytes);
  };
  auto count_of = [&](int c) {
    const uint32_t word = c < 2 ? hdr.x : (c < 4 ? hdr.y : (c < 6 ? hdr.z : hdr.w));
    return (int)((word >> ((c & 1) * 16)) & 0xffffu);
  };

  float4 st[4];
  load_tile(t_begin, st);
  load_lists(t_begin);
  store_tile(0, st);
  __syncthreads();

  const int hb = wave >> 3, hr0 = (wave & 7) * 32 + (lane >> 5);
  for (int t = t_begin; t < t_end; ++t) {
    const int b = (t - t_begin) & 1;
    const int tn = std::min(t + 1, t_end - 1);   // past the range: the same tile again, loaded and never used
    const char* buf = smem + b * kBufBytes;
    const char* more = overs + lists_of(t) * kOverBytes;   // blocks 1.. of the tile's lists
    int2 over = first[0];
    if (count_of(0) > kBlock) over = *reinterpret_cast<const int2*>(more);
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
      const int cnt = count_of(c);   // uniform in a quarter wave
      int longest = std::max(cnt, __shfl_xor(cnt, 16, 64));
      longest = __builtin_amdgcn_readfirstlane(std::max(longest, __shfl_xor(longest, 32, 64)));
      // a slot ahead: block 1 of the next list, where it has one
      int2 over_n = over;
      if (c + 1 < kSlots && count_of(c + 1 < kSlots ? c + 1 : c) > kBlock)
        over_n = *reinterpret_cast<const int2*>(more + (c + 1) * kOverBytes);
      int2 cur = first[c];
      for (int j0 = 0; j0 < longest; j0 += kBlock) {
        const int left = cnt - j0;
        if (left > 0) {
          int2 ahead = over;   // two blocks on
          if (left > 2 * kBlock) ahead = *reinterpret_cast<const int2*>(more + c * kOverBytes + (j0 + kBlock) * 8);
          col_group<0>(buf, i16 * 16, cur, acc[c]);
          if (left > kGroup) col_group<kGroup>(buf, i16 * 16, cur, acc[c]);
          if (left > 2 * kGroup) col_group<2 * kGroup>(buf, i16 * 16, cur, acc[c]);
          if (left > 3 * kGroup) col_group<3 * kGroup>(buf, i16 * 16, cur, acc[c]);
          cur = over;
          over = ahead;
        }
      }
      over = over_n;
    }
    load_tile(tn, st);
    {
      const float* a = reinterpret_cast<const float*>(buf) + hr0 * kSlab + hb * 32 + (lane & 31);
      const float* xh = strip + ((int64_t)t * kTile + hr0) * kStrip + (lane & 31);
#pragma unroll
      for (int kk = 0; kk < 16; ++kk)
        hacc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2 * kk * kSlab], xh[2 * kk * kStrip], hacc, 0, 0, 0);
    }
    store_tile(b ^ 1, st);
    load_lists(tn);
    __syncthreads();
  }

  // The heavy shares, merged in wave order: the dz buffers are free, so every wave parks its 16 accumulators in 4 KB
  // of its own, [wave][r][lane]; behind one barrier thread (wave, lane) sums, for two r of its half's 16, the eight
  // shares of lane `lane` from +0 in wave order (a sum of -0 shares stays +0, as a zeroed cell that is added to).
  float hsum[2];
  {
#pragma unroll
    for (int r = 0; r < 16; ++r) smemf[(wave * 16 + r) * 64 + lane] = hacc[r];
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = 2 * (wave & 7) + rr;
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) s += smemf[((hb * 8 + w) * 16 + r) * 64 + lane];
      hsum[rr] = s;
    }
    __syncthreads();
  }

  // the partial dw^T slab, transposed through LDS: out[n][k], pad columns zero, the bias sums behind it
  for (int i = tid; i < kBiasFloat + kSlab; i += kWgWaves * 64) smemf[i] = 0.f;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kSlots; ++c) {
    const int col = plan[kStrip + owner * kSlots + c];
    if (col >= 0 && col < K) {
      smemf[(4 * i16 + 0) * kTPitch + col] = acc[c].x;
      smemf[(4 * i16 + 1) * kTPitch + col] = acc[c].y;
      smemf[(4 * i16 + 2) * kTPitch + col] = acc[c].z;
      smemf[(4 * i16 + 3) * kTPitch + col] = acc[c].w;
    }
  }
  {   // a heavy column is nobody's light column: these cells are written once
    const int h = lane & 31;
    const int hc = h < kStrip - 1 ? plan[h] : -1;
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
      const int r = 2 * (wave & 7) + rr;
      const int nl = hb * 32 + 8 * (r / 4) + 4 * (lane >> 5) + (r % 4);
      if (h == kStrip - 1) smemf[kBiasFloat + nl] = hsum[rr];
      else if (hc >= 0 && hc < K) smemf[nl * kTPitch + hc] = hsum[rr];
    }
  }
  __syncthreads();
  for (int nn = wave; nn < kSlab; nn += kWgWaves) {
    if (n0 + nn < N) {
      float* dst = slabs + range * slab_stride + (int64_t)(n0 + nn) * lddw;
      for (int k = lane; k < lddw; k += 64) dst[k] = smemf[nn * kTPitch + k];
    }
  }
  if (bias_part && tid < kSlab && n0 + tid < N)
    bias_part[range * bias_stride + n0 + tid] = smemf[kBiasFloat + tid];
}

static int wgrad_compute_units() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  return cus;
}

// row tiles per range and the number of ranges (= slabs of the workspace): one workgroup per CU where the shape
// allows it, no range empty
static void wgrad_ranges(int64_t M, int N, int* per, int* ranges) {
  const int64_t tiles = (M + kTile - 1) / kTile;
  const int slabs = (N + kSlab - 1) / kSlab;
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(wgrad_compute_units() / slabs, tiles));
  *per = (int)((tiles + want - 1) / want);
  *ranges = (int)((tiles + *per - 1) / *per);
}

static bool wgrad_shape_ok(int K, int64_t lddw) { return K <= kWgMaxK && lddw <= kWgMaxK; }

}  // namespace itts

using namespace itts;

extern "C" int itts_sparse_cols_plan_ints(void) { return kPlanInts; }

extern "C" int itts_sparse_cols_layout(int64_t M, int K, int64_t out[3]) {
  ITTS_REQUIRE(out != nullptr, "null pointer");
  ITTS_REQUIRE(M >= 0 && K > 0 && K <= kWgMaxK, "bad sizes (K <= 512)");
  const ColsLayout l = cols_layout(M);
  out[0] = l.strip_off; out[1] = l.streams_off; out[2] = l.bytes;
  return ITTS_OK;
}

extern "C" int itts_sparse_cols_build(const float* d_x, int64_t ldx, int64_t M, int K, const int* d_plan, void* d_cols,
                                      void* stream) {
  ITTS_REQUIRE(d_plan && d_cols && (M == 0 || d_x), "null pointer");
  ITTS_REQUIRE(M >= 0 && K > 0 && K <= kWgMaxK && ldx >= K, "bad sizes (K <= 512)");
  ITTS_REQUIRE(aligned16(d_cols), "the column block must be 16-byte aligned");
  if (M == 0) return ITTS_OK;
  const ColsLayout l = cols_layout(M);
  const int parts = (K + 63) / 64;
  ITTS_REQUIRE(l.tiles * (parts + 1) < ((int64_t)1 << 31), "too many rows");
  char* base = static_cast<char*>(d_cols);
  hipLaunchKernelGGL(sparse_cols_build_kernel, dim3((unsigned)(l.tiles * (parts + 1))), dim3(256), 0,
                     as_stream(stream), reinterpret_cast<const uint32_t*>(d_x), ldx, M, K, parts, (int)l.tiles, d_plan,
                     reinterpret_cast<uint32_t*>(base + l.strip_off), base + l.streams_off);
  ITTS_LAUNCH_CHECK();
  g_wgrad_path[0].fetch_add(1, std::memory_order_relaxed);
  return ITTS_OK;
}

extern "C" int itts_sparse_cols_build_from_rows(const void* d_lists, int64_t M, int K_lists, int K, const int* d_plan,
                                                void* d_cols, void* stream) {
  ITTS_REQUIRE(d_plan && d_cols && (M == 0 || d_lists), "null pointer");
  ITTS_REQUIRE(M >= 0 && K > 0 && K <= kWgMaxK && K_lists >= K && K_lists <= 65535,
               "bad sizes (K <= 512, K <= K_lists <= 65535)");
  ITTS_REQUIRE(aligned16(d_cols) && aligned16(d_lists), "the column and list blocks must be 16-byte aligned");
  if (M == 0) return ITTS_OK;
  int64_t rows[4];   // counts, entries, pitch, bytes of the list block
  if (int rc = itts_sparse_rows_layout(M, K_lists, rows)) return rc;
  const ColsLayout l = cols_layout(M);
  ITTS_REQUIRE(l.tiles < ((int64_t)1 << 31), "too many rows");
  ITTS_HIP_CHECK(itts::allow_dynamic_lds((const void*)sparse_cols_from_rows_kernel, kFromRowsLdsBytes));
  const char* lists = static_cast<const char*>(d_lists);
  char* base = static_cast<char*>(d_cols);
  // the kernel reads two entries a lane: the pitch is a multiple of 16 entries, the entries start 16-byte aligned
  hipLaunchKernelGGL(sparse_cols_from_rows_kernel, dim3((unsigned)l.tiles), dim3(kFromRowsWaves * 64),
                     kFromRowsLdsBytes, as_stream(stream), reinterpret_cast<const int*>(lists + rows[0]),
                     reinterpret_cast<const int4*>(lists + rows[1]), rows[2] / 2, M, K, (int)l.tiles, d_plan,
                     reinterpret_cast<uint32_t*>(base + l.strip_off), base + l.streams_off);
  ITTS_LAUNCH_CHECK();
  g_wgrad_path[0].fetch_add(1, std::memory_order_relaxed);
  return ITTS_OK;
}

extern "C" int64_t itts_linear_bwd_weight_sparse_workspace_bytes(int64_t M, int N, int K, int64_t lddw) {
  if (M < 0 || N <= 0 || K <= 0 || lddw < K) return 0;
  const int64_t dense = itts_linear_bwd_weight_workspace_bytes(M, N, (int)lddw);
  if (M == 0 || !wgrad_shape_ok(K, lddw)) return dense;
  int per, ranges;
  wgrad_ranges(M, N, &per, &ranges);
  return std::max<int64_t>(dense, (int64_t)ranges * ((int64_t)N * lddw + N) * 4);
}

extern "C" int itts_linear_bwd_weight_sparse(const float* d_dz, int64_t lddz, const void* d_cols, const int* d_plan,
                                             const float* d_x, int64_t ldx, float* d_dw, int64_t lddw, float* d_db,
                                             int64_t M, int N, int K, void* d_workspace, int accumulate,
                                             void* stream) {
  ITTS_REQUIRE(d_dw && d_workspace && (M == 0 || (d_dz && d_x)), "null pointer");
  ITTS_REQUIRE(M >= 0 && N > 0 && K > 0 && lddz >= N && ldx >= K && lddw >= K, "bad sizes");
  ITTS_REQUIRE(lddw == K || ldx >= lddw, "x must be as wide as dw's rows (its pad columns zero)");
  const bool sparse = M > 0 && d_cols && d_plan && wgrad_shape_ok(K, lddw) && lddz % 4 == 0 && aligned16(d_dz) &&
                      aligned16(d_cols);
  if (!sparse) {   // decided on the host from the shape and the pointers: the dense product over dw's whole rows
    if (M > 0) g_wgrad_path[2].fetch_add(1, std::memory_order_relaxed);
    return itts_linear_bwd_weight(d_dz, lddz, d_x, ldx, d_dw, d_db, M, N, (int)lddw, d_workspace, accumulate, stream);
  }
  hipStream_t s = as_stream(stream);
  ITTS_HIP_CHECK(itts::allow_dynamic_lds((const void*)sparse_wgrad_kernel, kWgLdsBytes));
  const ColsLayout l = cols_layout(M);
  int per, ranges;
  wgrad_ranges(M, N, &per, &ranges);
  const int slabs_n = (N + kSlab - 1) / kSlab;
  ITTS_REQUIRE((int64_t)slabs_n * ranges < ((int64_t)1 << 31), "too many workgroups");
  const int64_t n = (int64_t)N * lddw;
  // db behind dw (the flat gradient arenas) and both lengths multiples of 4: one reduction serves both
  const bool merged = d_db && d_db == d_dw + n && N % 4 == 0 && n % 4 == 0;
  float* ws = static_cast<float*>(d_workspace);
  float* bias_part = !d_db ? nullptr : (merged ? ws + n : ws + (int64_t)ranges * n);
  const char* base = static_cast<const char*>(d_cols);
  hipLaunchKernelGGL(sparse_wgrad_kernel, dim3((unsigned)(slabs_n * ranges)), dim3(kWgWaves * 64), kWgLdsBytes, s, d_dz,
                     lddz, reinterpret_cast<const float*>(base + l.strip_off), base + l.streams_off, d_plan, ws,
                     merged ? n + N : n, (int)lddw, bias_part, merged ? n + N : (int64_t)N, M, N, K, (int)l.tiles, per,
                     ranges);
  ITTS_LAUNCH_CHECK();
  g_wgrad_path[1].fetch_add(1, std::memory_order_relaxed);
  if (merged) return reduce_slabs(ws, ranges, n + N, d_dw, accumulate, s);
  int rc = reduce_slabs(ws, ranges, n, d_dw, accumulate, s);
  if (rc || !d_db) return rc;
  return reduce_slabs(bias_part, ranges, (int64_t)N, d_db, accumulate, s);
}

extern "C" int itts_sparse_wgrad_counts(int64_t out[3]) {
  ITTS_REQUIRE(out != nullptr, "null pointer");
  for (int i = 0; i < 3; ++i) out[i] = g_wgrad_path[i].load(std::memory_order_relaxed);
  return ITTS_OK;
}
