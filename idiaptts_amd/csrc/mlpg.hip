// MLPG: maximum-likelihood parameter generation for the reference's three windows.
// Replaces MLPG.generation (idiaptts/misc/mlpg.py:94-127), i.e. the 62 python-level bandmat
// calls per utterance (build_poe :57-92, bla.solveh :125), by one call over all
// (utterance, dimension) pairs of a batch.
//
// The math (P x = b, banded Cholesky, two sweeps) is written once in mlpg_math.h.  One lane owns
// one (utterance, dimension); a wave owns 64 neighbouring dimensions so every row access is one
// coalesced 512-B segment.  This file is the only translation unit; the headers hold one solve form each:
//   mlpg_sweeps.h   mlpg_factor_kernel: the data-independent Cholesky factor, once per dimension, shared by all
//                   utterances (stops when it repeats); mlpg_kernel: the two sweeps frame by frame, short utterances
//   mlpg_ring.h     mlpg_ring_kernel: one pass, the right-hand side in LDS, from half a chip's worth of units
//   mlpg_stream.h   mlpg_prep / reduce / scan / solve: everything else, no wait anywhere: the backward contribution
//                   of a chunk is accumulated while walking forward (adjoint identity), a two-level scan gives every
//                   chunk its entry states, a second pass solves
//   mlpg_adjoint.h  the gradient with respect to the means (one more solve with the shared factor, then the three
//                   windows): mlpg_adjoint_kernel for short utterances (sequential, the windows inside the
//                   back-substitution), the stream form's solve + mlpg_adjoint_window_kernel for everything else
//   here            the choice of form, the override word, plans, the dispatcher and the C entry points
// (Rounds 2 and 3 also carried a four-pass chunked solve and a single-pass kernel with cross-workgroup
// waits; both measured slower -- DESIGN.md section 11c -- and left the library in round 4.)
//
// Roofline: HBM.  Algorithmic bytes per frame = 187*8 read + 63*8 written = 2000 B
// (SURVEY.md section 8d); measured traffic and rates: DESIGN.md section 11c.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "context.h"
#include "mlpg_adjoint.h"
#include "mlpg_math.h"
#include "mlpg_ring.h"
#include "mlpg_stream.h"
#include "mlpg_sweeps.h"

constexpr int MLPG_SEQ_BELOW = 194;   // utterances shorter than this take the sequential sweeps (three 64-frame chunks + tail)
constexpr int MLPG_RING_FROM = 128;     // (utterance, 64-dimension block) units from which the one-pass kernel takes over

using namespace itts;

extern "C" int64_t itts_mlpg_scratch_bytes(int64_t t_total, int dim) {
  if (t_total < 0 || dim <= 0) return 0;
  // 3 factor planes + device copy of the offsets (<= t_total + 1 entries, padded) + nconv
  return 3 * t_total * (int64_t)dim * 8 + (t_total + 2) * 8 + ((int64_t)dim * 4 + 16) / 8 * 8 + 8;
}

// float32 rows -> the float64 columns col0 .. col0 + 3 dim - 1 in a compact array (for the solves that read doubles)
__global__ void mlpg_widen_kernel(const float* __restrict__ src, int64_t ld, int col0, int cols, int64_t rows, double* __restrict__ dst) {
  const int64_t n = rows * cols;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    dst[i] = (double)src[r * ld + col0 + (i - r * cols)];
  }
}

// d_feat32 != nullptr: the input rows are float32 (d_feat unused); d_scratch then holds a [Ttot, 3 dim] float64
// array behind the usual scratch, for the batches that do not take the one-pass kernel
// What a call works out from the offsets alone, kept by a caller that solves over the same utterances again (the
// streams of one batch: mcep, lf0, bap; a trainer's fixed validation set): the checks, the longest length and -- for
// the one-pass kernel -- the (start, end) table in launch order, in page-locked memory of its own.  40-50 us of
// host time in front of a 230-us launch otherwise.
struct MlpgPlan {
  std::vector<int64_t> offsets;      // [n_utts + 1]
  int n_utts = 0;
  int64_t t_total = 0, t_max = 0;
  int64_t* table = nullptr;          // hipHostMalloc: (start, end) pairs, longest utterance first
};

static void mlpg_sorted_table(const int64_t* h_offsets, int n_utts, int64_t t_max, int64_t* out) {
  // utterances longest first, equal lengths in their own order: a counting sort over the lengths (a comparison sort
  // of 4 096 utterances was 0.15 ms of host time in front of a 2.8-ms launch)
  std::vector<int> order(n_utts);
  if (t_max <= (int64_t)1 << 20) {
    std::vector<int> start((size_t)t_max + 2, 0);
    for (int u = 0; u < n_utts; ++u) ++start[(size_t)(t_max - (h_offsets[u + 1] - h_offsets[u])) + 1];
    for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
    for (int u = 0; u < n_utts; ++u) order[start[(size_t)(t_max - (h_offsets[u + 1] - h_offsets[u]))]++] = u;
  } else {
    for (int u = 0; u < n_utts; ++u) order[u] = u;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) {
      return h_offsets[x + 1] - h_offsets[x] > h_offsets[y + 1] - h_offsets[y];
    });
  }
  for (int y = 0; y < n_utts; ++y) {
    out[2 * y] = h_offsets[order[y]];
    out[2 * y + 1] = h_offsets[order[y] + 1];
  }
}

static int mlpg_check_offsets(const int64_t* h_offsets, int n_utts, int64_t* t_max) {
  const int64_t t_total = h_offsets[n_utts];
  ITTS_REQUIRE(h_offsets[0] == 0 && t_total >= 0, "offsets must start at 0");
  for (int u = 0; u < n_utts; ++u)
    ITTS_REQUIRE(h_offsets[u + 1] >= h_offsets[u], "offsets must be non-decreasing");
  ITTS_REQUIRE(n_utts <= t_total + 1, "more utterances than frames");
  *t_max = 0;
  for (int u = 0; u < n_utts; ++u) *t_max = std::max(*t_max, h_offsets[u + 1] - h_offsets[u]);
  return ITTS_OK;
}

// ---- the choice of form (ITTS_MLPG_FORM_*, include/idiaptts_amd.h) --------------------------------------------------
// The override: solve | width << 4 | nt << 8 in one word, read once per call (a relaxed load; the environment was
// read by getenv once per process -- five calls were 2-3 us of every call).  The first use seeds it from the
// environment, so a later itts_mlpg_set_override is never overwritten by the seed.
static std::atomic<int>& mlpg_override() {
  static std::atomic<int> word{[] {
    const int solve = getenv("ITTS_MLPG_RING") ? ITTS_MLPG_FORM_RING : getenv("ITTS_MLPG_STREAM") ? ITTS_MLPG_FORM_STREAM : 0;
    const int width = getenv("ITTS_MLPG_NARROW") ? ITTS_MLPG_FORCE_OFF : getenv("ITTS_MLPG_WIDE") ? ITTS_MLPG_FORCE_ON : 0;
    const int nt = getenv("ITTS_MLPG_NO_NT") ? ITTS_MLPG_FORCE_OFF : 0;
    return solve | width << 4 | nt << 8;
  }()};
  return word;
}

static thread_local int t_mlpg_last_form = 0;

// The whole decision, from the shape and the override alone (the dispatcher and itts_mlpg_choose_form both call it).
static int mlpg_choose(int n_utts, int dim, int64_t t_max, int64_t t_total, bool f32, int ovr) {
  const int solve = ovr & 15, width = (ovr >> 4) & 15, nt = (ovr >> 8) & 15;
  const int f32_bits = f32 ? ITTS_MLPG_FORM_F32_ROWS | ITTS_MLPG_FORM_WIDENED_COPY : 0;
  if (t_max < MLPG_SEQ_BELOW) return ITTS_MLPG_FORM_SWEEPS | f32_bits;
  const int64_t units = (int64_t)n_utts * ((dim + RING_LANES - 1) / RING_LANES);
  // reduce -> scan -> solve with 16-frame chunks, two chunks per workgroup, input rows staged through LDS; from about
  // half a chip's worth of (utterance, 64 dimensions) units the one-pass kernel with the right-hand side in LDS
  // (mlpg_ring_kernel: a sequential sweep per unit -- 200 us for a 2 000-frame utterance however few there are -- so
  // small batches stay with the form above, which also divides an utterance among workgroups: 16 utterances 132
  // against 225 us, 64: 174 / 201, 256: 372 / 307, 4 096: 4 520 / 3 608)
  const bool ring = n_utts <= 65535 &&          // (an utterance per blockIdx.y)
                    (solve == ITTS_MLPG_FORM_RING || (solve != ITTS_MLPG_FORM_STREAM && units >= MLPG_RING_FROM));
  if (!ring) return ITTS_MLPG_FORM_STREAM | f32_bits;
  // two dimensions a lane in the helpers (half the memory instructions) where that is what the kernel waits for: float32
  // rows in batches of many rounds of workgroups -- 4 096 utterances 2.68 against 3.23 ms.  With float64 rows the
  // kernel moves 3.8 - 4.1 TB/s either way (3.62 / 3.61 ms), and at 256 utterances the exchange's extra arithmetic
  // costs 3 - 5 % (317 / 301 us; float32 231 / 223).  Even dim only.
  const bool wide = dim % 2 == 0 && width != ITTS_MLPG_FORCE_OFF && (width == ITTS_MLPG_FORCE_ON || (f32 && units >= 1024));
  if (f32) return ITTS_MLPG_FORM_RING | ITTS_MLPG_FORM_F32_ROWS | (wide ? ITTS_MLPG_FORM_WIDE : 0);
  if (wide) return ITTS_MLPG_FORM_RING | ITTS_MLPG_FORM_WIDE;
  // (float64 rows, y small enough to wait in the memory-side cache: input rows non-temporal -- see mlpg_ring.h, cache policy)
  const bool nt_in = nt != ITTS_MLPG_FORCE_OFF && (nt == ITTS_MLPG_FORCE_ON || t_total * dim * 8 <= (int64_t)192 << 20);
  return ITTS_MLPG_FORM_RING | (nt_in ? ITTS_MLPG_FORM_NT_IN : 0);
}

extern "C" int itts_mlpg_choose_form(int n_utts, int dim, int64_t t_max, int64_t t_total, int rows_f32) {
  ITTS_REQUIRE(n_utts >= 0 && dim > 0 && t_max >= 0 && t_total >= t_max, "bad sizes");
  return mlpg_choose(n_utts, dim, t_max, t_total, rows_f32 != 0, mlpg_override().load(std::memory_order_relaxed));
}

extern "C" int itts_mlpg_set_override(int solve, int width, int nt) {
  ITTS_REQUIRE(solve == 0 || solve == ITTS_MLPG_FORM_STREAM || solve == ITTS_MLPG_FORM_RING, "solve: 0, stream or ring");
  ITTS_REQUIRE(width >= 0 && width <= ITTS_MLPG_FORCE_ON, "width: 0, ITTS_MLPG_FORCE_OFF or ITTS_MLPG_FORCE_ON");
  ITTS_REQUIRE(nt >= 0 && nt <= ITTS_MLPG_FORCE_ON, "nt: 0, ITTS_MLPG_FORCE_OFF or ITTS_MLPG_FORCE_ON");
  mlpg_override().store(solve | width << 4 | nt << 8, std::memory_order_relaxed);
  return ITTS_OK;
}

extern "C" int itts_mlpg_get_override(int* solve, int* width, int* nt) {
  const int ovr = mlpg_override().load(std::memory_order_relaxed);
  if (solve) *solve = ovr & 15;
  if (width) *width = (ovr >> 4) & 15;
  if (nt) *nt = (ovr >> 8) & 15;
  return ITTS_OK;
}

extern "C" int itts_mlpg_last_form(void) {
  return t_mlpg_last_form;
}

// The instantiations of mlpg_ring_kernel, by the form bits that select them.
struct RingVariant { int bits; const void* kernel; };
static const RingVariant kRingVariants[] = {
  {ITTS_MLPG_FORM_F32_ROWS | ITTS_MLPG_FORM_WIDE, (const void*)mlpg_ring_kernel<float, true, false>},
  {ITTS_MLPG_FORM_F32_ROWS, (const void*)mlpg_ring_kernel<float, false, false>},
  {ITTS_MLPG_FORM_WIDE, (const void*)mlpg_ring_kernel<double, true, false>},
  {ITTS_MLPG_FORM_NT_IN, (const void*)mlpg_ring_kernel<double, false, true>},
  {0, (const void*)mlpg_ring_kernel<double, false, false>},
};

static int mlpg_generation_impl(const double* d_feat, const float* d_feat32, int64_t ld_feat, int col0, int dim,
                                const double* d_var, const int64_t* h_offsets, int n_utts,
                                double* d_out, int64_t ld_out, int ocol0, void* d_scratch,
                                void* stream, const MlpgPlan* plan = nullptr) {
  ITTS_REQUIRE(d_var && h_offsets && (n_utts == 0 || ((d_feat || d_feat32) && d_out && d_scratch)), "null pointer");
  ITTS_REQUIRE(dim > 0 && n_utts >= 0 && col0 >= 0 && ocol0 >= 0, "bad sizes");
  ITTS_REQUIRE(ld_feat >= col0 + 3 * (int64_t)dim && ld_out >= ocol0 + (int64_t)dim,
               "leading dimension too small");
  if (n_utts == 0) return ITTS_OK;
  const int64_t t_total = h_offsets[n_utts];
  int64_t t_max = 0;
  if (plan) {
    t_max = plan->t_max;
  } else {
    const int rc = mlpg_check_offsets(h_offsets, n_utts, &t_max);
    if (rc) return rc;
  }
  if (t_total == 0) return ITTS_OK;
  hipStream_t s = as_stream(stream);
  double* scratch = reinterpret_cast<double*>(d_scratch);
  int64_t* d_off = reinterpret_cast<int64_t*>(scratch + 3 * t_total * (int64_t)dim);
  int* d_nconv = reinterpret_cast<int*>(d_off + (t_total + 2));
  MlpgArgs a{d_feat, ld_feat, col0, dim, d_var, d_off, d_out, ld_out, ocol0, scratch, t_total, d_nconv};
  const int form = mlpg_choose(n_utts, dim, t_max, t_total, d_feat32 != nullptr, mlpg_override().load(std::memory_order_relaxed));
  t_mlpg_last_form = form;
  if (form & ITTS_MLPG_FORM_WIDENED_COPY) {
    // the other solves read doubles: widen the three column blocks once, behind the usual scratch
    double* wide = reinterpret_cast<double*>(reinterpret_cast<char*>(d_scratch) + itts_mlpg_scratch_bytes(t_total, dim));
    const int cols = 3 * dim;
    hipLaunchKernelGGL(mlpg_widen_kernel, dim3((unsigned)std::min<int64_t>((t_total * cols + 255) / 256, 8192)), dim3(256), 0, s,
                       d_feat32, ld_feat, col0, cols, t_total, wide);
    ITTS_LAUNCH_CHECK();
    a.feat = wide;
    a.ld_feat = cols;
    a.col0 = 0;
  }
  if ((form & ITTS_MLPG_FORM_SOLVE_MASK) == ITTS_MLPG_FORM_STREAM) {
    itts::ScratchScope scope(s);
    return mlpg_stream_launch(a, h_offsets, n_utts, dim, t_max, scope);
  }
  if ((form & ITTS_MLPG_FORM_SOLVE_MASK) == ITTS_MLPG_FORM_RING) {
    const RingVariant* variant = nullptr;
    for (const RingVariant& v : kRingVariants)
      if (v.bits == (form & (ITTS_MLPG_FORM_WIDE | ITTS_MLPG_FORM_F32_ROWS | ITTS_MLPG_FORM_NT_IN))) variant = &v;
    ITTS_REQUIRE(variant, "no one-pass kernel for this form");
    ITTS_HIP_CHECK(itts::allow_dynamic_lds(variant->kernel, RING_LDS_BYTES));
    itts::PinnedTable table;          // (nothing between here and the launch returns early: the slot goes back after it)
    const int64_t* bounds = plan ? plan->table : nullptr;
    if (!bounds) {
      std::vector<int64_t> host(2 * (size_t)n_utts);
      mlpg_sorted_table(h_offsets, n_utts, t_max, host.data());
      const int rc = itts::pinned_table_begin(host.data(), host.size() * sizeof(int64_t), &table);
      if (rc) return rc;
      bounds = static_cast<const int64_t*>(table.p);
    }
    a.offsets = nullptr;          // (the kernel has its bounds in the table)
    RingArgs g{a, bounds, (int)t_max, d_feat32};
    const dim3 rgrid((unsigned)((dim + RING_LANES - 1) / RING_LANES), (unsigned)n_utts), rblock(RING_THREADS);
    void* kernel_args[] = {&g};
    (void)hipLaunchKernel(variant->kernel, rgrid, rblock, kernel_args, RING_LDS_BYTES, s);
    const hipError_t launched = hipGetLastError();
    const int rc_table = plan && plan->table ? ITTS_OK : itts::pinned_table_end(&table, s);
    if (launched != hipSuccess) {
      itts::set_error(std::string("mlpg_ring_kernel: ") + hipGetErrorString(launched));
      return ITTS_E_HIP;
    }
    return rc_table;
  }
  {
    const int rc = itts::staged_upload(d_off, h_offsets, (size_t)(n_utts + 1) * sizeof(int64_t), s);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(mlpg_factor_kernel, dim3((dim + 63) / 64), dim3(64), 0, s, a, (int)t_max);
  ITTS_LAUNCH_CHECK();
  dim3 grid((dim + MLPG_LANES - 1) / MLPG_LANES, n_utts);
  hipLaunchKernelGGL(mlpg_kernel, grid, dim3(MLPG_LANES), 0, s, a, (int)t_max);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_mlpg_generation(const double* d_feat, int64_t ld_feat, int col0, int dim,
                                    const double* d_var, const int64_t* h_offsets, int n_utts,
                                    double* d_out, int64_t ld_out, int ocol0, void* d_scratch,
                                    void* stream) {
  t_mlpg_last_form = 0;
  ITTS_REQUIRE(n_utts == 0 || d_feat, "null pointer");
  return mlpg_generation_impl(d_feat, nullptr, ld_feat, col0, dim, d_var, h_offsets, n_utts, d_out, ld_out, ocol0, d_scratch, stream);
}

extern "C" int64_t itts_mlpg_scratch_bytes_f32(int64_t t_total, int dim) {
  if (t_total < 0 || dim <= 0) return 0;
  return itts_mlpg_scratch_bytes(t_total, dim) + t_total * 3 * (int64_t)dim * 8;
}

extern "C" int itts_mlpg_generation_f32(const float* d_feat, int64_t ld_feat, int col0, int dim,
                                        const double* d_var, const int64_t* h_offsets, int n_utts,
                                        double* d_out, int64_t ld_out, int ocol0, void* d_scratch,
                                        void* stream) {
  t_mlpg_last_form = 0;
  ITTS_REQUIRE(n_utts == 0 || d_feat, "null pointer");
  return mlpg_generation_impl(nullptr, d_feat, ld_feat, col0, dim, d_var, h_offsets, n_utts, d_out, ld_out, ocol0, d_scratch, stream);
}

// ---- prepared plans (see MlpgPlan) ----------------------------------------------------------------------------------
extern "C" int itts_mlpg_plan_create(const int64_t* h_offsets, int n_utts, void** plan_out) {
  ITTS_REQUIRE(h_offsets && plan_out && n_utts >= 0, "bad arguments");
  *plan_out = nullptr;
  std::unique_ptr<MlpgPlan> p(new MlpgPlan);
  p->n_utts = n_utts;
  p->offsets.assign(h_offsets, h_offsets + n_utts + 1);
  p->t_total = h_offsets[n_utts];
  if (n_utts > 0) {
    const int rc = mlpg_check_offsets(h_offsets, n_utts, &p->t_max);
    if (rc) return rc;
    ITTS_HIP_CHECK(hipHostMalloc((void**)&p->table, 2 * (size_t)n_utts * sizeof(int64_t), hipHostMallocDefault));
    mlpg_sorted_table(h_offsets, n_utts, p->t_max, p->table);
  }
  *plan_out = p.release();
  return ITTS_OK;
}

extern "C" void itts_mlpg_plan_destroy(void* plan) {
  MlpgPlan* p = static_cast<MlpgPlan*>(plan);
  if (!p) return;
  if (p->table) (void)hipHostFree(p->table);
  delete p;
}

extern "C" int64_t itts_mlpg_plan_frames(const void* plan) {
  return plan ? static_cast<const MlpgPlan*>(plan)->t_total : -1;
}

extern "C" int itts_mlpg_generation_planned(const void* plan, const void* d_feat, int feat_is_f32, int64_t ld_feat,
                                            int col0, int dim, const double* d_var, double* d_out, int64_t ld_out,
                                            int ocol0, void* d_scratch, void* stream) {
  const MlpgPlan* p = static_cast<const MlpgPlan*>(plan);
  t_mlpg_last_form = 0;
  ITTS_REQUIRE(p && (p->n_utts == 0 || d_feat), "null pointer");
  // (a launch reads the plan's table in place: the plan must outlive the work queued on `stream`)
  return mlpg_generation_impl(feat_is_f32 ? nullptr : static_cast<const double*>(d_feat),
                              feat_is_f32 ? static_cast<const float*>(d_feat) : nullptr, ld_feat, col0, dim, d_var,
                              p->offsets.data(), p->n_utts, d_out, ld_out, ocol0, d_scratch, stream, p);
}

// ---- the adjoint (mlpg_adjoint.h) -----------------------------------------------------------------------------------
extern "C" int64_t itts_mlpg_adjoint_scratch_bytes(int64_t t_total, int dim) {
  if (t_total < 0 || dim <= 0) return 0;
  // the forward's scratch (factor planes, offsets, nconv) + one [Ttot, dim] plane: the forward sweep's intermediate y
  // (sweeps) or z (stream)
  return itts_mlpg_scratch_bytes(t_total, dim) + t_total * (int64_t)dim * 8;
}

// The instantiations of mlpg_adjoint_kernel by (gradient in is float32, gradient out is float32).
static const void* const kAdjointKernels[2][2] = {
  {(const void*)mlpg_adjoint_kernel<double, double>, (const void*)mlpg_adjoint_kernel<double, float>},
  {(const void*)mlpg_adjoint_kernel<float, double>, (const void*)mlpg_adjoint_kernel<float, float>},
};

// The adjoint's own choice of form and override word (the forward's are not touched): sweeps under MLPG_SEQ_BELOW
// frames, the stream form from there; no ring form.  The override forces one of the two for any length.
static std::atomic<int> g_mlpg_adjoint_override{0};
static thread_local int t_mlpg_adjoint_last_form = 0;

static int mlpg_adjoint_choose(int64_t t_max, int ovr) {
  if (ovr) return ovr;
  return t_max < MLPG_SEQ_BELOW ? ITTS_MLPG_FORM_SWEEPS : ITTS_MLPG_FORM_STREAM;
}

extern "C" int itts_mlpg_adjoint_choose_form(int n_utts, int dim, int64_t t_max, int64_t t_total) {
  ITTS_REQUIRE(n_utts >= 0 && dim > 0 && t_max >= 0 && t_total >= t_max, "bad sizes");
  return mlpg_adjoint_choose(t_max, g_mlpg_adjoint_override.load(std::memory_order_relaxed));
}

extern "C" int itts_mlpg_adjoint_set_override(int form) {
  ITTS_REQUIRE(form == 0 || form == ITTS_MLPG_FORM_SWEEPS || form == ITTS_MLPG_FORM_STREAM, "form: 0, sweeps or stream");
  g_mlpg_adjoint_override.store(form, std::memory_order_relaxed);
  return ITTS_OK;
}

extern "C" int itts_mlpg_adjoint_get_override(void) {
  return g_mlpg_adjoint_override.load(std::memory_order_relaxed);
}

extern "C" int itts_mlpg_adjoint_last_form(void) {
  return t_mlpg_adjoint_last_form;
}

static int mlpg_adjoint_impl(const void* d_gout, int gout_is_f32, int64_t ld_gout, int gcol0, int dim,
                             const double* d_var, const int64_t* h_offsets, int n_utts,
                             void* d_gfeat, int gfeat_is_f32, int64_t ld_gfeat, int col0,
                             void* d_scratch, void* stream, const MlpgPlan* plan = nullptr) {
  t_mlpg_adjoint_last_form = 0;
  ITTS_REQUIRE(d_var && h_offsets, "null pointer");
  ITTS_REQUIRE(dim > 0 && n_utts >= 0 && gcol0 >= 0 && col0 >= 0, "bad sizes");
  ITTS_REQUIRE((dim + MLPG_ADJ_LANES - 1) / MLPG_ADJ_LANES <= 65535, "too many dimensions");
  ITTS_REQUIRE(ld_gout >= gcol0 + (int64_t)dim && ld_gfeat >= col0 + 3 * (int64_t)dim,
               "leading dimension too small");
  if (n_utts == 0) return ITTS_OK;
  const int64_t t_total = h_offsets[n_utts];
  int64_t t_max = 0;
  if (plan) {
    t_max = plan->t_max;
  } else {
    const int rc = mlpg_check_offsets(h_offsets, n_utts, &t_max);
    if (rc) return rc;
  }
  if (t_total == 0) return ITTS_OK;      // (a tensor without rows has no address: the pointers are looked at from here)
  ITTS_REQUIRE(d_gout && d_gfeat && d_scratch, "null pointer");
  ITTS_REQUIRE(t_max <= INT32_MAX, "utterance too long");
  hipStream_t s = as_stream(stream);
  double* scratch = reinterpret_cast<double*>(d_scratch);
  int64_t* d_off = reinterpret_cast<int64_t*>(scratch + 3 * t_total * (int64_t)dim);
  int* d_nconv = reinterpret_cast<int*>(d_off + (t_total + 2));
  double* d_y = reinterpret_cast<double*>(reinterpret_cast<char*>(d_scratch) + itts_mlpg_scratch_bytes(t_total, dim));
  MlpgArgs a{nullptr, 0, 0, dim, d_var, d_off, nullptr, 0, 0, scratch, t_total, d_nconv};
  MlpgAdjointArgs g{a, d_gout, ld_gout, gcol0, d_gfeat, ld_gfeat, col0, d_y};
  const int form = mlpg_adjoint_choose(t_max, g_mlpg_adjoint_override.load(std::memory_order_relaxed));
  t_mlpg_adjoint_last_form = form;
  if (form == ITTS_MLPG_FORM_STREAM) {
    itts::ScratchScope scope(s);
    return mlpg_adjoint_stream_launch(g, gout_is_f32 != 0, gfeat_is_f32 != 0, h_offsets, n_utts, t_max, scope);
  }
  {
    const int rc = itts::staged_upload(d_off, h_offsets, (size_t)(n_utts + 1) * sizeof(int64_t), s);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(mlpg_factor_kernel, dim3((dim + 63) / 64), dim3(64), 0, s, a, (int)t_max);
  ITTS_LAUNCH_CHECK();
  int t_max_arg = (int)t_max;
  void* kernel_args[] = {&g, &t_max_arg};
  const dim3 grid((unsigned)n_utts, (unsigned)((dim + MLPG_ADJ_LANES - 1) / MLPG_ADJ_LANES));
  ITTS_HIP_CHECK(hipLaunchKernel(kAdjointKernels[gout_is_f32 ? 1 : 0][gfeat_is_f32 ? 1 : 0], grid, dim3(MLPG_ADJ_LANES),
                                 kernel_args, 0, s));
  return ITTS_OK;
}

extern "C" int itts_mlpg_adjoint(const void* d_gout, int gout_is_f32, int64_t ld_gout, int gcol0, int dim,
                                 const double* d_var, const int64_t* h_offsets, int n_utts,
                                 void* d_gfeat, int gfeat_is_f32, int64_t ld_gfeat, int col0,
                                 void* d_scratch, void* stream) {
  return mlpg_adjoint_impl(d_gout, gout_is_f32, ld_gout, gcol0, dim, d_var, h_offsets, n_utts, d_gfeat, gfeat_is_f32,
                           ld_gfeat, col0, d_scratch, stream);
}

extern "C" int itts_mlpg_adjoint_planned(const void* plan, const void* d_gout, int gout_is_f32, int64_t ld_gout,
                                         int gcol0, int dim, const double* d_var, void* d_gfeat, int gfeat_is_f32,
                                         int64_t ld_gfeat, int col0, void* d_scratch, void* stream) {
  const MlpgPlan* p = static_cast<const MlpgPlan*>(plan);
  ITTS_REQUIRE(p, "null pointer");
  return mlpg_adjoint_impl(d_gout, gout_is_f32, ld_gout, gcol0, dim, d_var, p->offsets.data(), p->n_utts, d_gfeat,
                           gfeat_is_f32, ld_gfeat, col0, d_scratch, stream, p);
}
