// MLPG, the one-pass form: mlpg_ring_kernel.  Included by mlpg.hip only.
#pragma once
#include <type_traits>

#include "mlpg_math.h"

namespace itts {

// ---- one pass: the right-hand side never leaves the CU (round 5) ----------------------------------------------------
// A workgroup owns (utterance, 64 dimensions: all of them for the usual 60 + 1 + 1 streams).  Wave 0 walks the two
// sweeps frame by frame, a lane a dimension; the b / y / x rows it works on live in LDS -- a ring of RING_CAP frames x
// 64 doubles (147 KB) -- so that the recurrences' operands are LDS reads issued ahead of the chain (what mlpg_kernel
// pays per frame in memory latency is gone) and the input rows are read ONCE.  Seven helper waves work 24-frame
// segments around the sweep -- forward: the input rows of a segment a ring's length ahead -> b into the ring, after
// moving the y that occupied those slots (RING_CAP frames back) out to the output rows; backward: the finished
// segment's x out to the output rows, then the y of a ring's length further down back into the slots.  Progress words in
// LDS instead of barriers, no hand-off between workgroups, no scratch, ONE launch: the sweep derives the factor's
// moving head (the first 30 - 50 rows, until it repeats) itself while it walks them -- the same arithmetic as
// mlpg_factor_kernel, row by row -- and leaves the rows in the factor table for the way back.
//
// What shaped it (scripts/lat_lab, profiles/r5_mlpg_ring.md):
//  * a lone wave issues an instruction every 5 - 7 cycles whatever its width, so the sweep costs the same for 16
//    lanes as for 64: the first form of this kernel (16 dimensions x 1 152 frames a workgroup, the whole y of most
//    utterances in LDS) spent 4 x the sweep time of this one to save the y round trip.  Here y makes the trip (out and
//    back through the output rows, last in first out): 48 bytes per frame and dimension where the algorithm needs
//    32 and the three launch form moves 65;
//  * what a frame costs the sweep is its instruction COUNT: a segment that lies on the stationary factor altogether
//    is straight-line code, 4 instructions a frame; everything else (the head, the segment with the tail frames)
//    runs in ROLLED loops -- unrolled they were 40 KB of code that runs once a workgroup, every line of it an
//    instruction-cache miss behind the helpers' streams (40 us for the first segment);
//  * the CU has ONE memory pipeline: a load the sweep waits for queues behind whatever the seven helpers have asked
//    for (5 us on the way forward).  The sweep therefore does not wait for loads: the head's factor rows are derived on
//    the way forward; on the way back -- the helpers only store by then, a trip is the L2's 0.5 - 1 us -- they come
//    from the table twelve rows ahead of their use;
//  * every row of the factor's head is a frame off the straight-line path: what a solve takes followed the VARIANCES
//    (21 to 270 rows until the factor repeats) until the head's own cost was cut (last paragraph);
//  * the helpers' segment, row and edge arithmetic belongs on the scalar unit (wave number through readfirstlane).
// Arithmetic: mlpg_math.h's, as in every other form.
// Cache policy of the streams (input rows, x stores, y read back, y parked), measured with each of them non-temporal or
// not (every variant on one box, same variances): none of them matters at 4 096 utterances or with float32 rows;
// float64 rows at 256 utterances 258 -> 247 us with the INPUT rows non-temporal -- the y that is out (156 MB) then
// survives in the 256-MB memory-side cache until it comes back.  The kernel's NT_IN takes that; every other access is
// a plain load or store.
#define RING_LOAD_IN(p) (NT_IN ? __builtin_nontemporal_load(p) : *(p))
constexpr int RING_LANES = 64, RING_SEG = 24, RING_CAP = 288, RING_HELPERS = 7, RING_THREADS = 64 * (1 + RING_HELPERS);
constexpr int RING_LDS_BYTES = RING_CAP * RING_LANES * 8 + 128;     // + progress words
static_assert(RING_CAP % RING_SEG == 0 && RING_SEG % 8 == 0, "ring geometry");
struct RingArgs {
  MlpgArgs a;
  const int64_t* bounds;  // [workgroup rank][2]: first frame, end frame of its utterance (utterances longest first)
  int t_max;
  const float* feat32;    // the input rows when they are float32 (itts_mlpg_generation_f32): a.feat is unused then
};
// progress words in LDS (one writer each; release / acquire at workgroup scope)
enum RingWord : int {
  RING_W_FWD = 0,          // forward sweep: segments finished
  RING_W_HELPER_FWD = 1,   // + h: helper h, forward: its segments prepared (count)
  RING_W_BWD_BEGUN = 8,    // the backward sweep has begun
  RING_W_HELPER_BWD = 9,   // + h: helper h, backward: its segments stored / refilled (count)
  RING_W_BWD = 16,         // backward sweep: lowest segment finished (n_segments: none yet)
  RING_W_BOUNDS = 24,      // (behind the progress words: the utterance's two bounds, 16 bytes)
};
__device__ __forceinline__ void ring_post(int* w, int v) { __hip_atomic_store(w, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int ring_peek(const int* w) { return __hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }

// FT: the type of the input rows (double, or float: the network's own output type -- converted in the load, which is exact)
// WIDE: the helpers move two dimensions a lane and two rows an instruction (an even number of dimensions)
// NT_IN: the input rows are read with the non-temporal hint (see the cache policy above)
template <typename FT, bool WIDE, bool NT_IN>
__global__ __launch_bounds__(RING_THREADS) void mlpg_ring_kernel(RingArgs g) {
  extern __shared__ __attribute__((aligned(16))) char rsm[];
  double* ring = reinterpret_cast<double*>(rsm);          // [RING_CAP][64]
  int* prog = reinterpret_cast<int*>(rsm + RING_CAP * RING_LANES * 8);
  const MlpgArgs& a = g.a;
  const int blk = blockIdx.x;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  // the utterances' bounds are read in place from page-locked host memory (no copy on the stream in front of the
  // launch): one thread fetches this workgroup's pair -- one 16-byte load, one trip over the bus --, the others get it
  // through LDS
  int64_t* bounds = reinterpret_cast<int64_t*>(prog + RING_W_BOUNDS);
  if (tid == 0) {
    typedef int64_t Pair __attribute__((ext_vector_type(2)));
    const Pair b = reinterpret_cast<const Pair*>(g.bounds)[blockIdx.y];
    bounds[0] = b.x;
    bounds[1] = b.y;
  }
  if (tid < RING_W_BOUNDS) prog[tid] = 0;
  __syncthreads();
  const int64_t t0 = bounds[0];
  const int T = (int)(bounds[1] - t0);            // (frames of one utterance: 32 bits)
  if (T <= 0) return;
  const int D = a.dim;
  const int nseg = (T + RING_SEG - 1) / RING_SEG;
  constexpr int ring_segs = RING_CAP / RING_SEG;
  // slot of the first frame of segment sgm (the ring holds a whole number of segments: the frames of a segment sit in
  // consecutive slots)
  auto seg_slot = [](int sgm) { return (sgm % ring_segs) * RING_SEG; };
  const int dc = blk * RING_LANES + lane < D ? blk * RING_LANES + lane : D - 1;
  const int64_t plane = (int64_t)g.t_max * D;                 // the factor table: three planes of t_max rows

  if (wave != 0) {
    // ================= helper wave h: segments q = h, h + H, h + 2 H ..  (a lane: one dimension)
    // (the wave number through readfirstlane: segment numbers, row numbers and the edge tests are then the scalar
    // unit's work and the branches on them branches of the wave -- left as threadIdx arithmetic they were vector
    // selects around every load and every frame: 600 cycles a frame, 15 us a segment)
    const int h = wave - 1;
    const int hd = blk * RING_LANES + lane;
    const double hrv0 = 1.0 / a.var[dc], hrv1 = 1.0 / a.var[D + dc], hrv2 = 1.0 / a.var[2 * D + dc];
    const FT* hf = (std::is_same<FT, float>::value ? reinterpret_cast<const FT*>(g.feat32) : reinterpret_cast<const FT*>(a.feat)) +
                   t0 * a.ld_feat + a.col0 + dc;
    double* o = a.out + t0 * a.ld_out + a.ocol0 + dc;
    auto r1 = [&](int t) { return mlpg_rvar(t, T, hrv1); };
    auto r2 = [&](int t) { return mlpg_rvar(t, T, hrv2); };
    // ---- forward: input rows -> b into the ring, never more than a ring's length ahead of the sweep
    int mine = 0;
    // one segment; INNER: no frame of it is, or neighbours, an edge of the utterance (no row clamps, no edge variances)
    auto forward_segment = [&](int q, auto inner_tag) {
      constexpr bool INNER = decltype(inner_tag)::value;
      const int j0 = q * RING_SEG;
      double* base = ring + seg_slot(q) * RING_LANES + lane;
      // the whole segment's loads in flight together, and BEFORE the wait for its slots (registers are the only place
      // they need; seven helpers x 24 frames under way whatever the sweep is doing): the static column of rows j0 ..
      // j0 + 23, the delta and delta-delta columns of rows j0 - 1 .. j0 + 24 (each row serves as a frame's own and as
      // both its neighbours'), row numbers held inside the utterance
      double st[RING_SEG], d1[RING_SEG + 2], d2[RING_SEG + 2];
#pragma unroll
      for (int i = 0; i < RING_SEG + 2; ++i) {
        int r = j0 - 1 + i;
        if (!INNER) r = r < 0 ? 0 : (r < T ? r : T - 1);
        const FT* row = hf + (int64_t)r * a.ld_feat;
        d1[i] = (double)RING_LOAD_IN(row + D);
        d2[i] = (double)RING_LOAD_IN(row + 2 * D);
        if (i >= 1 && i <= RING_SEG) st[i - 1] = (double)RING_LOAD_IN(row);
      }
      while (q - ring_peek(prog + RING_W_FWD) >= ring_segs) __builtin_amdgcn_s_sleep(2);      // the sweep has left segment q - ring_segs
      if (j0 >= RING_CAP && hd < D) {                   // the y of frames j0 - RING_CAP .. leave the ring
#pragma unroll
        for (int i = 0; i < RING_SEG; ++i)
          if (INNER || j0 + i < T) o[(int64_t)(j0 + i - RING_CAP) * a.ld_out] = base[i * RING_LANES];
      }
#pragma unroll
      for (int i = 0; i < RING_SEG; ++i) {
        const int j = j0 + i;
        if (INNER || j < T) {
          double bj;
          if (INNER) {
            const double c0 = st[i] * hrv0, c2 = d2[i + 1] * hrv2;
            const double p1 = d1[i] * hrv1, p2 = d2[i] * hrv2;
            const double n1 = d1[i + 2] * hrv1, n2 = d2[i + 2] * hrv2;
            bj = mlpg_rhs(c0, p1, n1, p2, c2, n2);
          } else {
            const double c0 = st[i] * hrv0, c2 = d2[i + 1] * r2(j);
            const double p1 = j > 0 ? d1[i] * r1(j - 1) : 0.0, p2 = j > 0 ? d2[i] * r2(j - 1) : 0.0;
            const double n1 = j + 1 < T ? d1[i + 2] * r1(j + 1) : 0.0, n2 = j + 1 < T ? d2[i + 2] * r2(j + 1) : 0.0;
            bj = mlpg_rhs(c0, p1, n1, p2, c2, n2);
          }
          base[i * RING_LANES] = hd < D ? bj : 0.0;
        }
      }
      ++mine;
      if (lane == 0) ring_post(prog + RING_W_HELPER_FWD + h, mine);          // (a wave's LDS operations execute in order: the segment is in the ring)
    };
    // ---- the same with 16-byte accesses: a lane owns TWO dimensions (2 L, 2 L + 1 of the block; L = lane & 31) and a
    // memory instruction covers two rows (lanes 0 .. 31 the even row of a pair, 32 .. 63 the odd one): half the
    // memory instructions for the same bytes.  Pays where the instructions, not the bytes, are what the way forward
    // waits for: float32 rows at many rounds of workgroups (the host chooses; see the launch).  The rows a frame needs
    // from the other half of the wave -- its neighbours -- come over with v_permlane32_swap.
    typedef double V2d __attribute__((ext_vector_type(2), aligned(8)));       // (rows are 8-byte aligned, not 16)
    typedef FT V2f __attribute__((ext_vector_type(2), aligned(sizeof(FT))));
    const int wh = lane >> 5, wl = lane & 31;
    const int wd0 = blk * RING_LANES + 2 * wl;                   // this lane's dimensions wd0, wd0 + 1 (D even: both live or neither)
    const bool wlive = wd0 < D;
    const int wdc = wlive ? wd0 : 0;
    V2d wrv0, wrv1, wrv2;
    const FT* whf = nullptr;
    double* wo = nullptr;
    if constexpr (WIDE) {
      wrv0 = V2d{1.0 / a.var[wdc], 1.0 / a.var[wdc + 1]};
      wrv1 = V2d{1.0 / a.var[D + wdc], 1.0 / a.var[D + wdc + 1]};
      wrv2 = V2d{1.0 / a.var[2 * D + wdc], 1.0 / a.var[2 * D + wdc + 1]};
      whf = (std::is_same<FT, float>::value ? reinterpret_cast<const FT*>(g.feat32) : reinterpret_cast<const FT*>(a.feat)) +
            t0 * a.ld_feat + a.col0 + wdc;
      wo = a.out + t0 * a.ld_out + a.ocol0 + wdc;
    }
    auto widen = [](V2f v) { return V2d{(double)v.x, (double)v.y}; };
    // the other half's value of x in this lane (lanes < 32 get what lanes >= 32 hold and the other way round), as the
    // pair (lower half's view, upper half's view) the selections below pick from
    auto swap1 = [](double x, double& from_upper, double& from_lower) {
      const unsigned lo = (unsigned)__double2loint(x), hi = (unsigned)__double2hiint(x);
      const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
      const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
      // r[0]: lanes 32 .. 63 now hold the lower half's values; r[1]: lanes 0 .. 31 hold the upper half's
      from_lower = __hiloint2double((int)rh[0], (int)rl[0]);
      from_upper = __hiloint2double((int)rh[1], (int)rl[1]);
    };
    auto swap_halves = [&](V2d x, V2d& from_upper, V2d& from_lower) {
      double ux, uy, lx, ly;
      swap1(x.x, ux, lx);
      swap1(x.y, uy, ly);
      from_upper = V2d{ux, uy};
      from_lower = V2d{lx, ly};
    };
    auto forward_segment_wide = [&](int q, auto inner_tag) {
      constexpr bool INNER = decltype(inner_tag)::value;
      constexpr int NP = RING_SEG / 2;                 // row pairs of the segment: pair p = rows j0 + 2 p - 2, j0 + 2 p - 1
      const int j0 = q * RING_SEG;
      double* base = ring + seg_slot(q) * RING_LANES + 2 * wl;
      V2d st[NP], d1[NP + 2], d2[NP + 2];
#pragma unroll
      for (int p = 0; p < NP + 2; ++p) {
        int r = j0 - 2 + 2 * p + wh;
        if (!INNER) r = r < 0 ? 0 : (r < T ? r : T - 1);
        const FT* row = whf + (int64_t)r * a.ld_feat;
        d1[p] = widen(RING_LOAD_IN(reinterpret_cast<const V2f*>(row + D)));
        d2[p] = widen(RING_LOAD_IN(reinterpret_cast<const V2f*>(row + 2 * D)));
        if (p >= 1 && p <= NP) st[p - 1] = widen(RING_LOAD_IN(reinterpret_cast<const V2f*>(row)));
      }
      while (q - ring_peek(prog + RING_W_FWD) >= ring_segs) __builtin_amdgcn_s_sleep(2);      // the sweep has left segment q - ring_segs
      if (j0 >= RING_CAP && wlive) {                   // the y of frames j0 - RING_CAP .. leave the ring
#pragma unroll
        for (int k = 0; k < NP; ++k) {
          const int i = 2 * k + wh;
          if (INNER || j0 + i < T)
            *reinterpret_cast<V2d*>(wo + (int64_t)(j0 + i - RING_CAP) * a.ld_out) = *reinterpret_cast<const V2d*>(base + i * RING_LANES);
        }
      }
      // u[p] (delta: u1, delta-delta: u2): the entries of row j0 + 2 p - 3 + wh -- for the frame of pair p in this lane
      // (row j0 + 2 p - 2 + wh) the row before it, for the frame of pair p - 1 the row after it.  Formed pair by pair
      // and used at once (all of them held would be 112 registers): frame k = p - 2 wants u[p - 1] and u[p].
      V2d up1 = V2d{0.0, 0.0}, up2 = up1;              // pair p - 1 as the lower half sees the upper one (its odd row)
      V2d uq1 = up1, uq2 = up1;                        // u[p - 1]
#pragma unroll
      for (int p = 0; p < NP + 2; ++p) {
        V2d fu1, fl1, fu2, fl2;
        swap_halves(d1[p], fu1, fl1);
        swap_halves(d2[p], fu2, fl2);
        const V2d uc1 = wh ? fl1 : up1, uc2 = wh ? fl2 : up2;      // u[p] (p >= 1)
        up1 = fu1;
        up2 = fu2;
        if (p >= 2) {
          const int k = p - 2, i = 2 * k + wh, j = j0 + i;
          if (INNER || j < T) {
            V2d bj;
            if (INNER) {
              const V2d c0 = st[k] * wrv0, c2 = d2[k + 1] * wrv2;
              const V2d p1 = uq1 * wrv1, p2 = uq2 * wrv2;
              const V2d n1 = uc1 * wrv1, n2 = uc2 * wrv2;
              bj = mlpg_rhs(c0, p1, n1, p2, c2, n2);
            } else {
              const V2d zero = V2d{0.0, 0.0};
              auto e1 = [&](int t) { return mlpg_rvar(t, T, wrv1); };
              auto e2 = [&](int t) { return mlpg_rvar(t, T, wrv2); };
              const V2d c0 = st[k] * wrv0, c2 = d2[k + 1] * e2(j);
              const V2d p1 = j > 0 ? uq1 * e1(j - 1) : zero, p2 = j > 0 ? uq2 * e2(j - 1) : zero;
              const V2d n1 = j + 1 < T ? uc1 * e1(j + 1) : zero, n2 = j + 1 < T ? uc2 * e2(j + 1) : zero;
              bj = mlpg_rhs(c0, p1, n1, p2, c2, n2);
            }
            *reinterpret_cast<V2d*>(base + i * RING_LANES) = wlive ? bj : V2d{0.0, 0.0};
          }
        }
        uq1 = uc1;
        uq2 = uc2;
      }
      ++mine;
      if (lane == 0) ring_post(prog + RING_W_HELPER_FWD + h, mine);
    };
    for (int q = h; q < nseg; q += RING_HELPERS) {
      const bool inner = q >= 1 && q * RING_SEG + RING_SEG <= T - 2;
      if constexpr (WIDE) {
        if (inner) forward_segment_wide(q, std::true_type{});
        else forward_segment_wide(q, std::false_type{});
      } else {
        if (inner) forward_segment(q, std::true_type{});
        else forward_segment(q, std::false_type{});
      }
    }
    // ---- backward: x of a finished segment out, then the y of a ring's length further down back into its slots
    int fetched = 0;
    // this wave's segments, highest first
    int qtop = nseg - 1;
    while (qtop >= 0 && qtop % RING_HELPERS != h) --qtop;
    while (ring_peek(prog + RING_W_BWD_BEGUN) == 0) __builtin_amdgcn_s_sleep(2);
    for (int q = qtop; q >= 0; q -= RING_HELPERS) {
      const int j0 = q * RING_SEG;
      double* base = ring + seg_slot(q) * RING_LANES + lane;
      const int qf = q - ring_segs;          // its frames went out on the way forward iff frame + RING_CAP < T
      // (the bytes read here were written in the forward phase, before RING_W_BWD_BEGUN was posted -- no later store of this
      // workgroup touches them before this load -- so the loads need not wait for the sweep either)
      if constexpr (WIDE) {
        constexpr int NP = RING_SEG / 2;
        double* wbase = ring + seg_slot(q) * RING_LANES + 2 * wl;
        V2d yw[NP];
        if (qf >= 0 && wlive) {
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            const int j = qf * RING_SEG + 2 * k + wh;
            yw[k] = (j + RING_CAP < T) ? *reinterpret_cast<const V2d*>(wo + (int64_t)j * a.ld_out) : V2d{0.0, 0.0};
          }
        }
        while (ring_peek(prog + RING_W_BWD) > q) __builtin_amdgcn_s_sleep(2);     // the backward sweep has finished segment q
        if (wlive) {
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            const int i = 2 * k + wh;
            if (j0 + i < T) *reinterpret_cast<V2d*>(wo + (int64_t)(j0 + i) * a.ld_out) = *reinterpret_cast<const V2d*>(wbase + i * RING_LANES);
          }
          if (qf >= 0) {
#pragma unroll
            for (int k = 0; k < NP; ++k) {
              const int i = 2 * k + wh;
              if (qf * RING_SEG + i + RING_CAP < T) *reinterpret_cast<V2d*>(wbase + i * RING_LANES) = yw[k];
            }
          }
        }
      } else {
      double yv[RING_SEG];
      if (qf >= 0 && hd < D) {
#pragma unroll
        for (int k = 0; k < RING_SEG; ++k) {
          const int j = qf * RING_SEG + k;
          yv[k] = (j + RING_CAP < T) ? o[(int64_t)j * a.ld_out] : 0.0;
        }
      }
      while (ring_peek(prog + RING_W_BWD) > q) __builtin_amdgcn_s_sleep(2);     // the backward sweep has finished segment q
      if (hd < D) {
#pragma unroll
        for (int k = 0; k < RING_SEG; ++k)
          if (j0 + k < T) o[(int64_t)(j0 + k) * a.ld_out] = base[k * RING_LANES];
        if (qf >= 0) {
#pragma unroll
          for (int k = 0; k < RING_SEG; ++k) {
            const int j = qf * RING_SEG + k;
            if (j + RING_CAP < T) base[k * RING_LANES] = yv[k];
          }
        }
      }
      }
      ++fetched;
      if (lane == 0) ring_post(prog + RING_W_HELPER_BWD + h, fetched);
    }
    return;
  }

  // ================= wave 0: the two sweeps, a lane a dimension
  const double v0 = a.var[dc], v1 = a.var[D + dc], v2 = a.var[2 * D + dc];
  const MlpgPrec<int> prec{T, 1.0 / v0, 1.0 / v1, 1.0 / v2};
  double* fd = a.scratch + dc;
  double* fl1 = fd + plane;
  double* fl2 = fl1 + plane;
  // the shared factor's view of the variances ("T = infinity"), as mlpg_factor_block has it: rows 2 .. are one row
  const double pjj_in = prec.row<true>(2).pjj, pj1_in = prec.row<true>(2).pj1;
  const double pj2_in = prec.row<true>(0).pj2;          // (every row's)
  const int n_shared = T >= 3 ? T - 2 : 0;
  // the factor: rows 0 .. ncvmax derived on the way forward (a lane's entries stay put from its own row of repetition
  // on: mlpg_factor_block's rule), the stationary entries in three registers from there
  double sd = 0.0, sl1 = 0.0, sl2 = 0.0;
  bool lane_settled = false;             // this lane's factor has repeated: (sd, sl1, sl2) hold
  bool settled = false;                  // every lane's has
  int ncvmax = 0x7fffffff;               // the row at which the last lane's did
  MlpgTail tail;                         // frames T - 2, T - 1
  double l1p = 0.0, l2p = 0.0, cprev = 0.0, y1 = 0.0, y2 = 0.0;
  double* lane_ring = ring + lane;

  __builtin_amdgcn_s_setprio(3);         // (the SIMD is shared with a helper wave: the sweep goes first)
  auto relaxed = [](const int* w) { return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };

  // ---- forward
  int hsel = 0, hcnt = 0, slot = 0;       // segment sgm: helper sgm % H, its (sgm / H + 1)-th; first ring slot
  int seen = relaxed(prog + RING_W_HELPER_FWD);
  for (int sgm = 0; sgm < nseg; ++sgm) {
    // (what the sweep needs to know about the segment after this one -- is it in the ring yet? -- is asked for before
    // the chain and looked at after it)
    if (seen <= hcnt)
      while (ring_peek(prog + RING_W_HELPER_FWD + hsel) <= hcnt) __builtin_amdgcn_s_sleep(1);   // segment sgm is in the ring
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int hsel_n = hsel + 1 == RING_HELPERS ? 0 : hsel + 1, hcnt_n = hsel + 1 == RING_HELPERS ? hcnt + 1 : hcnt;
    seen = relaxed(prog + RING_W_HELPER_FWD + hsel_n);
    const int j0 = sgm * RING_SEG;
    const int jend = j0 + RING_SEG < T ? j0 + RING_SEG : T;
    double* sl = lane_ring + slot * RING_LANES;         // slot of frame j: sl[(j - j0) * 64]
    if (settled && j0 >= ncvmax + 2 && j0 + RING_SEG <= n_shared) {
      // the whole segment on the stationary factor, two stationary frames behind it: straight-line code, the 24
      // right-hand sides read at once, the chain, the writes
      double v[RING_SEG];
#pragma unroll
      for (int i = 0; i < RING_SEG; ++i) v[i] = sl[i * RING_LANES];
#pragma unroll
      for (int i = 0; i < RING_SEG; ++i) {
        const double y = (v[i] - sl1 * y1 - sl2 * y2) * sd;
        sl[i * RING_LANES] = y;
        y2 = y1;
        y1 = y;
      }
    } else {
      // the head (the factor still moves: derived here, row by row, and left in the table for the way back), the
      // frames between it and the first whole stationary segment, the segment with the two re-derived tail frames:
      // a rolled loop, the right-hand side of the frame after asked for first
      double nb = sl[0];
#pragma unroll 1
      for (int j = j0; j < jend; ++j) {
        const int jn = j + 1 < jend ? j + 1 : j;
        const double nb_n = sl[(jn - j0) * RING_LANES];
        double dd = sd, l1 = sl1, l2 = sl2;                    // dd holds 1 / L[j,j]
        if (j >= n_shared) {
          mlpg_chol_step<false>(prec.row<false>(j), l1p, l2p, cprev, dd, l1, l2);
          tail.put(j, T, dd, l1, l2);
        } else if (!settled) {
          if (!lane_settled) {
            // (P's entries are those of row 2 from there on: the same expressions on the same values)
            MlpgRow p{pjj_in, pj1_in, pj2_in};
            if (j < 2) {
              p.pjj = prec.row<true>(j).pjj;
              p.pj1 = prec.row<true>(j).pj1;
            }
            mlpg_chol_step<true>(p, l1p, l2p, cprev, dd, l1, l2);
            if (mlpg_factor_settled(j, l1, l2, l1p, l2p, cprev)) {
              lane_settled = true;
              sd = dd; sl1 = l1; sl2 = l2;
            }
          }
          fd[(int64_t)j * D] = dd;           // (every workgroup leaves the same values here)
          fl1[(int64_t)j * D] = l1;
          fl2[(int64_t)j * D] = l2;
          if (__all(lane_settled)) {
            settled = true;
            ncvmax = j;
          }
        }
        const double y = (nb - l1p * y1 - l2p * y2) * dd;
        sl[(j - j0) * RING_LANES] = y;
        l2p = cprev;
        l1p = l1;
        cprev = l2;
        y2 = y1;
        y1 = y;
        nb = nb_n;
      }
    }
    if (lane == 0) ring_post(prog + RING_W_FWD, sgm + 1);
    hsel = hsel_n; hcnt = hcnt_n; slot = slot + RING_SEG == RING_CAP ? 0 : slot + RING_SEG;
  }
  // the helpers have prepared everything (the sweep consumed it); their counters start again for the way back
  // ---- backward: L^T x = y, segments from the last to the first
  // the head's rows: 0 .. ncvmax - 1 where the factor settled (row ncvmax on is the registers'), else every shared row
  const int head_rows = settled ? ncvmax : n_shared;
  const int head_last = settled ? ncvmax : n_shared - 1;      // the last row of the table (settled: the stationary one)
  if (lane == 0) {
    ring_post(prog + RING_W_BWD, nseg);          // lowest finished segment: none yet
    ring_post(prog + RING_W_BWD_BEGUN, 1);
  }
  double x1 = 0.0, x2 = 0.0;
  // segment sgm's y is still in the ring, or comes back with the helper that stores segment qs = sgm + ring_segs: helper
  // qs % H, whose count stands at (nseg - 1 - qs) / H + 1 after that segment (it takes its segments from the top)
  slot = seg_slot(nseg - 1);
  int bq = 0, bh = 0, bneed = 0;           // for the segment at hand: bq >= 0: it has to wait, for helper bh to count bneed
  auto counters_for = [&](int sgm) {
    const int qs = sgm + ring_segs;
    bh = qs % RING_HELPERS;
    bq = nseg - 1 - qs;
    bneed = bq >= 0 ? bq / RING_HELPERS + 1 : 0;
  };
  counters_for(nseg - 1);
  int seen_b = bq >= 0 ? relaxed(prog + RING_W_HELPER_BWD + bh) : 0;
  // The head's rows come back from the table -- this workgroup's own rows of it, a sweep's length old.  A trip to the
  // L2 is 0.5 - 1 us, five to ten frames of this sweep: a segment that reaches into the head (and holds none of the
  // two tail frames) is therefore straight-line code in two halves of twelve rows, the rows of a half (1 / L[j,j] and
  // L[j+1,j]; L[j+2,j] is pj2 times the first, as it was formed) asked for while the half before it is worked; frames
  // of it above the head read the table's last row, which holds the stationary entries.  (Until late in round 5 the
  // helpers put heads of up to 56 rows into free slots of the ring for a rolled loop to read: slower than this for 50
  // rows -- 2.84 against 2.76 ms at 4 096 utterances -- and a progress protocol of its own.)
  constexpr int HALF = RING_SEG / 2;
  double ud[HALF], u1[HALF], wd[HALF], w1[HALF];        // upper half (rows j0 + 23 .. j0 + 12), lower half (j0 + 11 .. j0)
  auto table_seg = [&](int sg) {
    return sg >= 0 && sg * RING_SEG < head_rows && sg * RING_SEG + RING_SEG <= n_shared;
  };
  auto load_upper = [&](int sg) {
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
      const int row = sg * RING_SEG + RING_SEG - 1 - i;
      const int64_t r = (int64_t)(row < head_last ? row : head_last) * D;
      ud[i] = fd[r];
      u1[i] = fl1[r];
    }
  };
  auto load_lower = [&](int sg) {
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
      const int row = sg * RING_SEG + HALF - 1 - i;
      const int64_t r = (int64_t)(row < head_last ? row : head_last) * D;
      wd[i] = fd[r];
      w1[i] = fl1[r];
    }
  };
  for (int sgm = nseg - 1; sgm >= 0; --sgm) {
    if (bq >= 0 && seen_b < bneed)
      while (ring_peek(prog + RING_W_HELPER_BWD + bh) < bneed) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (sgm > 0) {
      counters_for(sgm - 1);
      seen_b = bq >= 0 ? relaxed(prog + RING_W_HELPER_BWD + bh) : 0;
    }
    const int j0 = sgm * RING_SEG;
    const int jtop = (j0 + RING_SEG < T ? j0 + RING_SEG : T) - 1;
    double* sl = lane_ring + slot * RING_LANES;
    const bool cur_tab = table_seg(sgm), next_tab = table_seg(sgm - 1);
    if (!cur_tab && next_tab) load_upper(sgm - 1);
    if (cur_tab) {
      load_lower(sgm);
      double v[HALF];
#pragma unroll
      for (int i = 0; i < HALF; ++i) v[i] = sl[(RING_SEG - 1 - i) * RING_LANES];
#pragma unroll
      for (int i = 0; i < HALF; ++i) {
        const double x = (v[i] - u1[i] * x1 - (pj2_in * ud[i]) * x2) * ud[i];
        sl[(RING_SEG - 1 - i) * RING_LANES] = x;
        x2 = x1;
        x1 = x;
      }
      if (next_tab) load_upper(sgm - 1);
#pragma unroll
      for (int i = 0; i < HALF; ++i) v[i] = sl[(HALF - 1 - i) * RING_LANES];
#pragma unroll
      for (int i = 0; i < HALF; ++i) {
        const double x = (v[i] - w1[i] * x1 - (pj2_in * wd[i]) * x2) * wd[i];
        sl[(HALF - 1 - i) * RING_LANES] = x;
        x2 = x1;
        x1 = x;
      }
    } else if (j0 >= head_rows && j0 + RING_SEG <= n_shared) {
      double v[RING_SEG];
#pragma unroll
      for (int i = 0; i < RING_SEG; ++i) v[i] = sl[(RING_SEG - 1 - i) * RING_LANES];
#pragma unroll
      for (int i = 0; i < RING_SEG; ++i) {
        const double x = (v[i] - sl1 * x1 - sl2 * x2) * sd;
        sl[(RING_SEG - 1 - i) * RING_LANES] = x;
        x2 = x1;
        x1 = x;
      }
    } else {
      // rolled, as on the way forward (the segment with the tail frames; head rows in it -- an utterance shorter than
      // the head + a segment -- from the table, a row ahead)
      auto fetch = [&](int j, double& qd, double& q1, double& q2) {
        qd = sd; q1 = sl1; q2 = sl2;
        if (j >= n_shared) {
          tail.get(j, T, qd, q1, q2);
        } else if (j < head_rows) {
          qd = fd[(int64_t)j * D]; q1 = fl1[(int64_t)j * D]; q2 = fl2[(int64_t)j * D];
        }
      };
      double ny = sl[(jtop - j0) * RING_LANES], cd, c1, c2;
      fetch(jtop, cd, c1, c2);
#pragma unroll 1
      for (int j = jtop; j >= j0; --j) {
        const int jn = j - 1 >= j0 ? j - 1 : j;
        const double ny_n = sl[(jn - j0) * RING_LANES];
        double nd, n1, n2;
        fetch(jn, nd, n1, n2);
        const double x = (ny - c1 * x1 - c2 * x2) * cd;
        sl[(j - j0) * RING_LANES] = x;
        x2 = x1;
        x1 = x;
        ny = ny_n; cd = nd; c1 = n1; c2 = n2;
      }
    }
    if (lane == 0) ring_post(prog + RING_W_BWD, sgm);
    slot = slot == 0 ? RING_CAP - RING_SEG : slot - RING_SEG;
  }
}
#undef RING_LOAD_IN

}  // namespace itts
