// First dense layer on a sparse input for gfx950.  Layer 0 of the acoustic model reads min-max-normalised question
// vectors: binary answers plus a few numeric columns, 7-10 % non-zeros, and (x - min) / range keeps a zero an exact
// zero.  The dense product multiplies by those zeros; here every row of x becomes a list of its (k, value) pairs once
// per batch (sparse_rows_build_kernel), and the forward product walks the lists against a slab of w^T held in LDS
// (sparse_linear_fwd_kernel): per non-zero one 16-byte LDS read and four fmaf give four outputs.
//   * roofline: instruction issue and LDS reads side by side.  A list slot of four rows costs a wave four vector
//     instructions (the slab address, an add that carries the DPP broadcast of the entry's byte offset; the broadcast
//     of the value; two packed fmaf) and one ds_read_b128 (4 LDS cycles), and the walk runs to the longest of four
//     lists.  No wave waits for memory inside an ordinary group: what a group needs is requested a group ahead, and
//     the wait for it leaves the wave's own store of y in flight ("Load schedule and slot").
//   * what does not depend on the density: the slab fill (w read along k, 16 bytes a lane where w's rows allow it),
//     the store of y and the activation.
#include <algorithm>
#include <atomic>
#include <utility>

#include "activations.h"
#include "common.h"
#include "dropout.h"

namespace itts {

constexpr int kSparseMaxK = 512;      // the LDS slab holds (K + 1) x 64 floats: 131 KB of the CU's 160 KB
constexpr int kSlabCols = 64;         // output columns of a workgroup
constexpr int kFwdWaves = 16;         // one workgroup per CU (LDS), four waves per SIMD
constexpr int kRowsPerWave = 4;       // a quarter wave per row: 16 lanes x 4 columns
constexpr int kStep = 8;              // list slots per trip of the walk; the build pads every list to whole trips
constexpr int kFetch = 16;            // list entries per load: one per lane of a quarter wave
constexpr int kAhead = 48;            // entries of every row that are requested a group of rows ahead of their walk
constexpr int kAheadFetches = kAhead / kFetch;
constexpr int kSlabRowBytes = kSlabCols * 4;
constexpr int kFillTrips = kSparseMaxK / 4 / kFwdWaves;   // 16-byte loads of a lane in the slab fill
static_assert(kAhead % kFetch == 0 && kFetch == 2 * kStep, "the walk takes a fetch as two trips");

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef int intx2 __attribute__((ext_vector_type(2)));

static std::atomic<int64_t> g_sparse_path[3];

struct ListLayout {
  int64_t counts_off, entries_off, pitch, bytes;
};

static ListLayout list_layout(int64_t M, int K) {
  ListLayout l;
  l.counts_off = 16;
  l.entries_off = 16 + (M * 4 + 15) / 16 * 16;
  l.pitch = ((int64_t)K + kFetch - 1) / kFetch * kFetch;   // a load of the walk never leaves its row
  l.bytes = l.entries_off + M * l.pitch * 8;
  return l;
}

// One wave per row, 256 columns per trip: the four loads of a trip go out together, then each 64-column group
// appends its non-zeros behind the ones before it (ballot + prefix count: ascending k without any sorting).  Behind
// the row's count the list is filled up to a multiple of kStep with neutral entries (k = K, value +0): the forward
// walk takes kStep slots per trip and needs no mask inside one, its slab has an all-zero row K.
__global__ __launch_bounds__(256) void sparse_rows_build_kernel(const uint32_t* __restrict__ x, int64_t ldx, int64_t M,
                                                                int K, int* __restrict__ counts,
                                                                int2* __restrict__ entries, int64_t pitch,
                                                                unsigned long long* __restrict__ record) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), wn = (int64_t)gridDim.x * 4;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long total = 0, most = 0;
  for (int64_t m = w0; m < M; m += wn) {
    const uint32_t* row = x + m * ldx;
    int2* out = entries + m * pitch;
    int cnt = 0;
    for (int k0 = 0; k0 < K; k0 += 256) {
      uint32_t bits[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + 64 * u + lane;
        bits[u] = k < K ? row[k] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool nz = (bits[u] & 0x7fffffffu) != 0u;   // +-0.0 out; NaN and denormals stay (no float compare)
        const unsigned long long mask = __ballot(nz);
        if (nz) out[cnt + __popcll(mask & below)] = make_int2(k0 + 64 * u + lane, (int)bits[u]);
        cnt += __popcll(mask);
      }
    }
    if (lane < ((kStep - cnt % kStep) % kStep)) out[cnt + lane] = make_int2(K, 0);   // neutral up to a whole trip
    if (lane == 0) counts[m] = cnt;
    total += (unsigned long long)cnt;
    most = std::max(most, (unsigned long long)cnt);
  }
  if (record && lane == 0 && total) {
    atomicAdd(&record[0], total);
    atomicMax(&record[1], most);
  }
}

// Slot J of the 16 list entries a quarter wave holds, entry j in its lane j, e.x already the byte offset of slab row
// k (slab_offsets): the DPP row broadcast hands lane J's (offset, value) to the quarter's 16 lanes, which read their
// 16 bytes of the slab row and do four fmaf.  Four VALU instructions: the offset's broadcast rides on the add of the
// lane's own offset (v_add_u32_dpp), the value's is a v_mov_b32_dpp, and two v_pk_fma_f32.  row_newbcast writes every
// lane, so the broadcasts need no defined `old`: bound_ctrl spares the v_mov that would zero it.
template <int J>
__device__ __forceinline__ void walk_slot(const char* slab, int lane_off, int2 e, float4& acc) {
  const int off = __builtin_amdgcn_update_dpp(0, e.x, 0x150 + J, 0xf, 0xf, true);   // row_newbcast:J
  const float v = __int_as_float(__builtin_amdgcn_update_dpp(0, e.y, 0x150 + J, 0xf, 0xf, true));
  const float4 wk = *reinterpret_cast<const float4*>(slab + (off + lane_off));
  acc.x = fmaf(v, wk.x, acc.x); acc.y = fmaf(v, wk.y, acc.y);
  acc.z = fmaf(v, wk.z, acc.z); acc.w = fmaf(v, wk.w, acc.w);
}
template <int FIRST, int... U>
__device__ __forceinline__ void walk_trip(const char* slab, int lane_off, int2 e, float4& acc,
                                          std::integer_sequence<int, U...>) {
  (walk_slot<FIRST + U>(slab, lane_off, e, acc), ...);
}
// the 16 entries of one fetch: k -> byte offset of slab row k, once per fetched entry
__device__ __forceinline__ int2 slab_offsets(int2 e) { return make_int2(e.x * kSlabRowBytes, e.y); }
// the two trips of a fetch, for a quarter whose list has `left` entries from this fetch's first on
__device__ __forceinline__ void walk_fetch(const char* slab, int lane_off, int2 e, int left, float4& acc) {
  if (left > 0) walk_trip<0>(slab, lane_off, e, acc, std::make_integer_sequence<int, kStep>());
  if (left > kStep) walk_trip<kStep>(slab, lane_off, e, acc, std::make_integer_sequence<int, kStep>());
}

// Workgroup = (64-column slab of w^T in LDS, row range); wave = four rows at a time, one per quarter wave; lane = four
// adjacent output columns of its quarter's row.  A quarter reads 16 entries of its row's list per load, entry j into
// lane j, and a DPP row broadcast hands entry j to its 16 lanes when slot j's turn comes, so k and the value sit in
// VGPRs and nothing has to be made wave-uniform (with every lane loading the entry itself the vector memory path
// moves 16 times the bytes and sets the kernel's time).  Per list slot a lane forms the slab address, reads 16 bytes
// and does four fmaf (two packed ones).  The neutral entries that fill a list's last trip read the slab's extra
// all-zero row K with a zero value: acc + 0 * 0.  The slab's rows are 64 floats apart, so the four rows a
// ds_read_b128 touches all start on bank 0 and every 16 lanes the hardware serves together cover the 64 banks once,
// whatever the four k are.  The walk runs to the longest of the four lists in trips of kStep slots, and a quarter
// whose list has ended sits the trips out.  The counts and the first kAhead entries of the next four rows are
// requested before the current rows are walked and waited for behind the current rows' store, by a wait that leaves
// that store in flight; only rows longer than kAhead fetch inside their walk, one fetch of kFetch entries ahead.  One
// fmaf chain per output, in ascending k, from +0; the bias is added last.
// (A list entry with k > K would read LDS out of range, which returns zeros; the lists come from the build.)
// DR: the dropout rule of the dense layers on the output (dropout.h: a lane's four columns are one Philox call), or
// NoDrop, which carries nothing.
template <int AF, class DR = NoDrop>
__global__ __launch_bounds__(kFwdWaves * 64) void sparse_linear_fwd_kernel(
    const int* __restrict__ counts, const int2* __restrict__ entries, int64_t pitch, const float* __restrict__ w,
    const float* __restrict__ bias, float* __restrict__ y, int64_t ldy, int64_t M, int N, int K, int act, int ranges,
    int store_cols, int wide_out, int wide_w, DR dr) {
  extern __shared__ float4 slab4[];   // [K + 1][16] float4
  float* slab = reinterpret_cast<float*>(slab4);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int n0 = (int)(blockIdx.x / ranges) * kSlabCols;
  const int range = (int)(blockIdx.x % ranges);
  const int64_t per = (M + ranges - 1) / ranges;
  const int64_t m_begin = range * per, m_end = std::min<int64_t>(M, m_begin + per);
  const int q = lane >> 4, c4 = (lane & 15) * 4;   // this lane's row of the group and its first column in the slab

  // slab[k][c] = w[n0 + c][k]: a lane per column, the waves take turns at k (each lane walks along its own row of w,
  // whose cache lines the other waves' turns reuse).  A wave load touches 64 lines, one per lane, whatever its
  // width, so with 16-byte rows of w a lane takes four k at a time: a quarter of the line requests, all of a wave's
  // loads in flight together, and four ds_write_b32 into consecutive slab rows (the lanes stay consecutive in a row:
  // conflict free).  Rows of w that are not 16-byte aligned keep the dword loop; the slab is the same either way.
  {
    const bool col_ok = n0 + lane < N;
    const float* wr = w + (int64_t)(col_ok ? n0 + lane : 0) * K;
    if (wide_w) {
      const float4* wr4 = reinterpret_cast<const float4*>(wr);
      const int K4 = K >> 2;
      float4 v[kFillTrips];
#pragma unroll
      for (int u = 0; u < kFillTrips; ++u) {
        const int j = wave + u * kFwdWaves;
        v[u] = (col_ok && j < K4) ? wr4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < kFillTrips; ++u) {
        const int j = wave + u * kFwdWaves;
        if (j < K4) {
          float* row = slab + 4 * j * kSlabCols + lane;
          row[0] = v[u].x; row[kSlabCols] = v[u].y; row[2 * kSlabCols] = v[u].z; row[3 * kSlabCols] = v[u].w;
        }
      }
    } else {
      for (int k = wave; k < K; k += kFwdWaves) slab[k * kSlabCols + lane] = col_ok ? wr[k] : 0.f;
    }
    if (wave == 0) slab[K * kSlabCols + lane] = 0.f;
  }

  // rows behind the range re-read the last row and are never used: no branch around a load
  auto row_of = [&](int64_t group) { return m_begin + (group * kRowsPerWave + q); };
  const int i16 = lane & 15;
  const int last_fetch = (int)pitch - kFetch;   // a fetch never leaves its row: a short pitch re-reads its last block
  auto fetch = [&](int64_t m, int j0) {
    return entries[std::min<int64_t>(m, M - 1) * pitch + (std::min(j0, last_fetch) + i16)];
  };
  // What a group of four rows needs before its walk: the counts and the first kAhead entries of every row, requested
  // before the group in front of it is walked.  The four loads are hidden from the compiler's wait counting: counted
  // by the compiler, the wait for them is a vmcnt(0) (paths with different numbers of loads meet before it), which
  // also waits for the y store issued behind them.  Vector memory operations retire in order, so wait_ahead<KEEP>
  // names the registers (nothing reads or moves them between the request and the wait) and leaves only the KEEP
  // operations issued behind the requests in flight.  Every load and store the compiler counts itself -- the fetches
  // of a row longer than kAhead, the stores -- is issued behind the requests of its group, so its own waits hold.
  struct Ahead {
    int cnt;
    intx2 e[kAheadFetches];
  };
  static_assert(kAheadFetches == 3, "request_ahead and wait_ahead name three fetches");
  auto request_ahead = [&](int64_t group, Ahead& a) {
    const int64_t m = std::min<int64_t>(row_of(group), M - 1);
    const int* pc = counts + m;
    const int2* pe = entries + m * pitch + i16;
    const int2 *p0 = pe, *p1 = pe + std::min(kFetch, last_fetch), *p2 = pe + std::min(2 * kFetch, last_fetch);
    asm volatile("global_load_dword %0, %1, off" : "=v"(a.cnt) : "v"(pc) : "memory");
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(a.e[0]) : "v"(p0) : "memory");
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(a.e[1]) : "v"(p1) : "memory");
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(a.e[2]) : "v"(p2) : "memory");
  };
  auto wait_ahead = [&](auto keep, Ahead& a) {
    // (the s_nop: a 16-byte store may sit right in front, whose data registers the code behind the wait rewrites)
    asm volatile("s_nop 1\n\ts_waitcnt vmcnt(%4)"
                 : "+v"(a.cnt), "+v"(a.e[0]), "+v"(a.e[1]), "+v"(a.e[2])
                 : "n"(decltype(keep)::value)
                 : "memory");
  };
  int64_t group = wave;
  Ahead next;
  request_ahead(group, next);
  __syncthreads();

  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  const int n = n0 + c4;
  if (bias) {
    if (n < N) bv.x = bias[n];
    if (n + 1 < N) bv.y = bias[n + 1];
    if (n + 2 < N) bv.z = bias[n + 2];
    if (n + 3 < N) bv.w = bias[n + 3];
  }
  const char* slab_bytes = reinterpret_cast<const char*>(slab4);
  const int lane_off = i16 * 16;
  // (the bias is used here so that the compiler waits for it here, and not at its uses in every group's epilogue)
  asm volatile("" ::"v"(bv.x), "v"(bv.y), "v"(bv.z), "v"(bv.w));
  wait_ahead(std::integral_constant<int, 0>{}, next);   // nothing is known to lie behind the first group's requests

  // WIDE: y's rows are 16-byte aligned and a lane's four columns are stored whole or not at all (store_cols is a
  // multiple of four then).  The store is a buffer store that every wave issues exactly once per group, outside any
  // branch -- a lane with nothing to store carries an offset beyond the buffer, which the hardware drops -- so exactly
  // one store lies behind a group's requests when the next group is about to start, and the wait there, vmcnt(1),
  // leaves it in flight: no wave waits for its own output.  The buffer is this range's rows of y; the host keeps a
  // range below 2 GB.
  // Not WIDE (a pitch or pointer of y that is not 16-byte aligned): up to four dword stores a lane, behind branches, so
  // their number is not known and the wait is a full one (vmcnt(0)), which also waits for the stores.
  auto run = [&](auto wide) {
    constexpr bool WIDE = decltype(wide)::value;
    const int64_t range_rows = std::max<int64_t>(m_end - m_begin, 1);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
        y + m_begin * ldy, 0, WIDE ? (int)(((range_rows - 1) * ldy + store_cols) * 4) : 0, 0x00020000);
    for (; m_begin + group * kRowsPerWave < m_end; group += kFwdWaves) {
      const int64_t m = row_of(group);
      const Ahead cur = next;
      request_ahead(group + kFwdWaves, next);
      const int cnt = m < m_end ? cur.cnt : 0;
      int longest = std::max(cnt, __shfl_xor(cnt, 16, 64));
      longest = __builtin_amdgcn_readfirstlane(std::max(longest, __shfl_xor(longest, 32, 64)));
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      // the first kAhead entries, from registers; a quarter whose list has ended sits the trips out
      auto walk_ahead = [&]() {
#pragma unroll
        for (int f = 0; f < kAheadFetches; ++f)
          if (f * kFetch < longest)
            walk_fetch(slab_bytes, lane_off, slab_offsets(make_int2(cur.e[f].x, cur.e[f].y)), cnt - f * kFetch, acc);
      };
      if (longest <= kAhead) {
        walk_ahead();   // the ordinary group: no wait for vector memory between its requests and its store
      } else {
        // Rows longer than kAhead: the fetches behind the first kAhead entries are loads the compiler counts, the
        // first requested here, the others one fetch ahead of their walk, each waited for before its walk.  This is a
        // branch of its own, with its own copy of the walk above, and every path through it uses every register it
        // loads into (`landed`): a load that could be pending where the two branches meet again, or at the next
        // group, puts a full wait into the ordinary group's walk.
        auto landed = [](int2 e) { asm volatile("" ::"v"(e.x), "v"(e.y)); };
        int2 more = fetch(m, kAhead);
        walk_ahead();
        int j0 = kAhead;
        for (; j0 + kFetch < longest; j0 += kFetch) {
          const int2 nxt = fetch(m, j0 + kFetch);
          landed(more);
          walk_fetch(slab_bytes, lane_off, slab_offsets(more), cnt - j0, acc);
          more = nxt;
        }
        landed(more);
        walk_fetch(slab_bytes, lane_off, slab_offsets(more), cnt - j0, acc);
      }
      float4 o;
      o.x = n < N ? act_fwd_af<AF>(acc.x + bv.x, act) : 0.f;
      o.y = n + 1 < N ? act_fwd_af<AF>(acc.y + bv.y, act) : 0.f;
      o.z = n + 2 < N ? act_fwd_af<AF>(acc.z + bv.z, act) : 0.f;
      o.w = n + 3 < N ? act_fwd_af<AF>(acc.w + bv.w, act) : 0.f;
      if constexpr (DR::on) {
        const uint4x dw = dr.words(m, n);
        o.x = dr.apply(o.x, dw.w[0]); o.y = dr.apply(o.y, dw.w[1]);
        o.z = dr.apply(o.z, dw.w[2]); o.w = dr.apply(o.w, dw.w[3]);
      }
      if constexpr (WIDE) {
        const bool stores = m < m_end && n + 4 <= store_cols;
        const uint32_t vo = stores ? (uint32_t)(((m - m_begin) * ldy + n) * 4) : 0xfffffff0u;
        floatx4 ov = {o.x, o.y, o.z, o.w};
        __builtin_amdgcn_raw_buffer_store_b128(ov, yrs, vo, 0, 0);
        wait_ahead(std::integral_constant<int, 1>{}, next);
      } else {
        if (m < m_end) {
        float* yr = y + m * ldy + n;
        if (n < store_cols) yr[0] = o.x;
        if (n + 1 < store_cols) yr[1] = o.y;
        if (n + 2 < store_cols) yr[2] = o.z;
        if (n + 3 < store_cols) yr[3] = o.w;
        }
        wait_ahead(std::integral_constant<int, 0>{}, next);
      }
    }
  };
  if (wide_out) run(std::true_type{});
  else run(std::false_type{});
}

}  // namespace itts

using namespace itts;

extern "C" int itts_sparse_rows_layout(int64_t M, int K, int64_t out[4]) {
  ITTS_REQUIRE(out != nullptr, "null pointer");
  ITTS_REQUIRE(M >= 0 && K > 0 && K <= 65535, "bad sizes (K <= 65535)");
  const ListLayout l = list_layout(M, K);
  out[0] = l.counts_off; out[1] = l.entries_off; out[2] = l.pitch; out[3] = l.bytes;
  return ITTS_OK;
}

extern "C" int itts_sparse_rows_build(const float* d_x, int64_t ldx, int64_t M, int K, void* d_lists, int want_record,
                                      void* stream) {
  ITTS_REQUIRE(d_lists && (M == 0 || d_x), "null pointer");
  ITTS_REQUIRE(M >= 0 && K > 0 && K <= 65535 && ldx >= K, "bad sizes (K <= 65535)");
  ITTS_REQUIRE(aligned16(d_lists), "the list block must be 16-byte aligned");
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(d_lists);
  if (want_record) ITTS_HIP_CHECK(hipMemsetAsync(base, 0, 16, s));
  if (M == 0) return ITTS_OK;
  const ListLayout l = list_layout(M, K);
  const unsigned grid = (unsigned)std::min<int64_t>((M + 3) / 4, 8192);
  hipLaunchKernelGGL(sparse_rows_build_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(d_x), ldx,
                     M, K, reinterpret_cast<int*>(base + l.counts_off), reinterpret_cast<int2*>(base + l.entries_off),
                     l.pitch, want_record ? reinterpret_cast<unsigned long long*>(base) : nullptr);
  ITTS_LAUNCH_CHECK();
  g_sparse_path[0].fetch_add(1, std::memory_order_relaxed);
  return ITTS_OK;
}

static int fwd_compute_units() {
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

template <int AF, class DR = NoDrop>
static int launch_sparse_fwd(const void* d_lists, const float* d_w, const float* d_b, float* d_y, int64_t ldy, int64_t M,
                             int N, int K, int act, hipStream_t s, const DR& dr = DR()) {
  ITTS_HIP_CHECK(itts::allow_dynamic_lds((const void*)sparse_linear_fwd_kernel<AF, DR>, (kSparseMaxK + 1) * kSlabCols * 4));
  const ListLayout l = list_layout(M, K);
  const char* base = static_cast<const char*>(d_lists);
  const int slabs = (N + kSlabCols - 1) / kSlabCols;
  // one workgroup per CU where the shape allows it; a range is worth its slab fill from about 64 rows on
  int64_t ranges = std::max<int64_t>(1, std::min<int64_t>(fwd_compute_units() / slabs, (M + 63) / 64));
  // the pad columns inside a 16-byte row pitch are written as zeros, as the dense epilogue does
  const bool wide_out = (ldy % 4 == 0) && aligned16(d_y) && ldy < (int64_t(1) << 28);
  // the 16-byte stores address a range's rows of y with 32-bit byte offsets: more ranges where y is that large
  if (wide_out) ranges = std::max(ranges, (M * ldy * 4 >> 31) + 1);
  const int store_cols = wide_out ? (int)std::min<int64_t>((N + 3) / 4 * 4, ldy) : N;
  hipLaunchKernelGGL((sparse_linear_fwd_kernel<AF, DR>), dim3((unsigned)(slabs * ranges)), dim3(kFwdWaves * 64),
                     (size_t)(K + 1) * kSlabCols * 4, s, reinterpret_cast<const int*>(base + l.counts_off),
                     reinterpret_cast<const int2*>(base + l.entries_off), l.pitch, d_w, d_b, d_y, ldy, M, N, K, act,
                     (int)ranges, store_cols, wide_out ? 1 : 0, (K % 4 == 0 && aligned16(d_w)) ? 1 : 0, dr);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

// DR: NoDrop behind itts_linear_fwd_sparse, DropRule (the rule of the dense layers, on the output) behind its _dropout
// form
template <class DR>
static int linear_fwd_sparse(const void* d_lists, const float* d_x, int64_t ldx, const float* d_w, const float* d_b,
                             float* d_y, int64_t ldy, int64_t M, int N, int K, int act, hipStream_t s, const DR& dr) {
  const char* const entry = DR::on ? "itts_linear_fwd_sparse_dropout" : "itts_linear_fwd_sparse";
  ITTS_REQUIRE_AS(entry, d_w && (M == 0 || (d_lists && d_x && d_y)), "null pointer");
  ITTS_REQUIRE_AS(entry, M >= 0 && N > 0 && K > 0 && K <= 65535 && ldx >= K && ldy >= N, "bad sizes");
  ITTS_REQUIRE_AS(entry, act >= ITTS_ACT_NONE && act <= ITTS_ACT_HARDSIGMOID, "unknown activation");
  if (M == 0) return ITTS_OK;
  if (K > kSparseMaxK) {   // the slab does not fit: the dense product, decided from the shape alone
    g_sparse_path[2].fetch_add(1, std::memory_order_relaxed);
    return itts::linear_fwd(d_x, ldx, d_w, d_b, d_y, ldy, M, N, K, act, s, dr);
  }
  g_sparse_path[1].fetch_add(1, std::memory_order_relaxed);
  if (act_family(act) == AF_EXT) return launch_sparse_fwd<AF_EXT, DR>(d_lists, d_w, d_b, d_y, ldy, M, N, K, act, s, dr);
  return launch_sparse_fwd<AF_BASE, DR>(d_lists, d_w, d_b, d_y, ldy, M, N, K, act, s, dr);
}

extern "C" int itts_linear_fwd_sparse(const void* d_lists, const float* d_x, int64_t ldx, const float* d_w,
                                      const float* d_b, float* d_y, int64_t ldy, int64_t M, int N, int K, int act,
                                      void* stream) {
  return linear_fwd_sparse(d_lists, d_x, ldx, d_w, d_b, d_y, ldy, M, N, K, act, as_stream(stream), NoDrop{});
}

extern "C" int itts_linear_fwd_sparse_dropout(const void* d_lists, const float* d_x, int64_t ldx, const float* d_w,
                                              const float* d_b, float* d_y, int64_t ldy, int64_t M, int N, int K,
                                              int act, double p, uint64_t seed, uint32_t salt, int64_t row_offset,
                                              void* stream) {
  ITTS_REQUIRE_DROP_P(p);
  if (p == 0.0)
    return linear_fwd_sparse(d_lists, d_x, ldx, d_w, d_b, d_y, ldy, M, N, K, act, as_stream(stream), NoDrop{});
  return linear_fwd_sparse(d_lists, d_x, ldx, d_w, d_b, d_y, ldy, M, N, K, act, as_stream(stream),
                           make_drop_rule(p, seed, salt, row_offset));
}

extern "C" int itts_sparse_path_counts(int64_t out[3]) {
  ITTS_REQUIRE(out != nullptr, "null pointer");
  for (int i = 0; i < 3; ++i) out[i] = g_sparse_path[i].load(std::memory_order_relaxed);
  return ITTS_OK;
}
