// Raw-waveform targets: the discretized mixture-of-logistics loss with its gradient in one launch
// (loss/DiscretizedMixturelogisticLoss.py of the reference), the mu-law companding and one-hot targets of
// data_preparation/audio/RawWaveformLabelGen.py, and misc/utils.py's sample_linearly.
//
// The loss.  x is [B, 3K, T] (logits, means, log-scales), lanes run along t as in xent.hip's strided form, one lane
// per frame, the K mixtures in ascending order inside the lane: a frame's bits depend on that frame alone.  Per
// mixture, with s = max(r, log_scale_min) of the raw log-scale r, i = e^-s, c = y - mean, h = 1 / (num_classes - 1),
//     u = i (c + h),   v = i (c - h),   m = i c,   d = u - v = 2 h i  (exact, and > 0),
// the reference's four branches and their derivatives by the mean and by s (sg = sigmoid, th(x) = tanh(x / 2),
// sp = softplus):
//     y < -0.999     L = log sg(u) = -sp(-u)            dL/dmean = -i sg(-u)             dL/ds = -u sg(-u)
//     y >  0.999     L = log(1 - sg(v)) = -sp(v)        dL/dmean =  i sg(v)              dL/ds =  v sg(v)
//     delta > 1e-5   L = log delta                      dL/dmean =  i (th(u) + th(v)) / 2
//                                                       dL/ds = v (th(u) + th(v)) / 2 - d sg(-u) / (sg(-v) E)
//     else           L = m - s - 2 sp(m) - log((num_classes - 1) / 2)
//                                                       dL/dmean =  i th(m)              dL/ds = m th(m) - 1
// delta = sg(u) - sg(v) is never formed as a difference: sg(u) - sg(v) = sg(u) sg(-v) E with E = 1 - e^-d = -expm1(-d),
// three positive factors, so log delta = -sp(-u) - sp(v) + log E keeps full relative precision where two float32
// sigmoids would cancel (delta ~ 1e-5 from two values near 1 or 0 leaves two digits).  The same identity gives the
// derivative: sg'(u) - sg'(v) = delta (sg(-v) - sg(u)), so delta divides out of dL/dmean, and sg(u) - sg(-v) =
// (th(u) + th(v)) / 2 with th from expm1: no 1 - small for a wide logistic; where y lies well inside the bin of a
// narrow one (th(u) > 1/2, th(v) < -1/2) the same quantity is taken from the tails, sg(v) - sg(-u), since the two
// tanh would cancel against each other.  h is carried as two floats: u and v are e^-s, up to 1e14, times c +- h,
// and where c +- h cancels the rounding of h alone (2e-10) would decide the result.  Branches are selected, never
// blended with cond * a + (1 - cond) * b: an overflow in a branch not taken cannot reach the result.
//
// Then q_k = L_k + log_softmax(logit)_k, l = -logsumexp_k q_k (+ sum_k max(0, -r_k - log num_classes) with hinge, on
// the raw log-scales), and with the responsibilities p_k = exp(q_k - lse):
//     dl/dlogit_k = softmax_k - p_k,   dl/dmean_k = -p_k dL_k/dmean,
//     dl/dr_k = -p_k dL_k/ds [r_k >= log_scale_min] - [hinge_k > 0].
// The lane keeps q_k and the two derivatives of its K mixtures in LDS, [3][K][lanes] floats (lane-contiguous: no bank
// conflicts), not in registers: K is a run-time value up to 64, and 192 live floats a lane would leave one wave a
// SIMD.  A workgroup has 256 lanes up to K = 16, 128 up to 32, 64 up to 64, which holds the block at 48 KiB: three
// workgroups a CU for every K.  The logits are read three times (maximum, sum, gradient), twice from the caches.
//
// Rows of weight 0 are not read.  w l is added in double: the lanes of a workgroup by the butterfly and wave by wave,
// the workgroups by a second launch in one fixed order.  No float atomics: repeated calls give identical bits.
#include <algorithm>
#include <math.h>
#include <vector>

#include "common.h"
#include "context.h"
#include "rawwave.h"

namespace itts {
namespace {

constexpr int MOL_MAX_K = 64;
constexpr int64_t RW_MAX_GRID_X = (1 << 24) - 1;
constexpr int RW_MAX_GRID_Y = 65535;
constexpr int RW_THREADS = 256;

int mol_threads(int K) { return K <= 16 ? 256 : K <= 32 ? 128 : 64; }
int64_t mol_chunks(int64_t T, int threads) { return (T + threads - 1) / threads; }

// everything the branches need of one argument x, from e^-|x| - 1 = expm1(-|x|)
struct Sig {
  float pos, neg;       // sigmoid(x), sigmoid(-x)
  float sp, sn;         // softplus(x), softplus(-x)
  float th;             // tanh(x / 2) = sigmoid(x) - sigmoid(-x)
};

__device__ __forceinline__ Sig sig_of(float x) {
  const float ax = fabsf(x);
  const float em = expm1f(-ax);         // in (-1, 0]
  const float e = 1.f + em;             // e^-|x|
  const float den = 2.f + em;           // 1 + e^-|x|
  const float big = 1.f / den, small = e / den;
  const float lg = log1pf(e);
  const float t = -em / den;
  Sig r;
  const bool p = x >= 0.f;
  r.pos = p ? big : small;
  r.neg = p ? small : big;
  r.sp = (p ? ax : 0.f) + lg;
  r.sn = (p ? 0.f : ax) + lg;
  r.th = p ? t : -t;
  return r;
}

struct MolArgs {
  const float* x;
  const float* y;
  const float* w;
  float* elem;
  float* grad;
  double* partial;              // [B][chunks]
  int64_t T, Tn;                // frames of the tensors / of the loss (T - shift)
  int K, shift, hinge;
  float h, hl, h2;              // 1 / (num_classes - 1) as two floats (h + hl), and twice h
  float lsm;                    // log_scale_min
  float log_nc, log_half;       // log(num_classes), log((num_classes - 1) / 2)
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void mol_kernel(MolArgs a) {
  extern __shared__ float keep[];       // [3][K][THREADS]: q, dL/dmean, dL/ds (0 below the clamp)
  __shared__ double red[16];
  const int tid = threadIdx.x;
  const int K = a.K;
  const int64_t t = (int64_t)blockIdx.x * THREADS + tid;
  const int64_t b = blockIdx.y;
  const bool have = t < a.Tn;
  const int64_t r = b * a.Tn + t;
  const int64_t base = b * 3 * K * a.T + t;
  const float wr = have ? a.w[r] : 0.f;
  const bool live = have && wr != 0.f;  // rows of weight 0 may hold anything: never read
  float* kq = keep + tid;
  float* km = keep + (int64_t)K * THREADS + tid;
  float* ks = keep + (int64_t)2 * K * THREADS + tid;
  float l = 0.f;
  if (live) {
    const float* xl = a.x + base;                        // logits
    const float* xm = xl + (int64_t)K * a.T;             // means
    const float* xs = xm + (int64_t)K * a.T;             // log-scales
    const float y = a.y[b * a.T + t + a.shift];
    float lmax = -INFINITY;
    for (int k = 0; k < K; ++k) lmax = fmaxf(lmax, xl[(int64_t)k * a.T]);
    float lsum = 0.f;
    for (int k = 0; k < K; ++k) lsum += expf(xl[(int64_t)k * a.T] - lmax);
    const float llog = logf(lsum);
    const bool low = y < -0.999f, high = y > 0.999f;
    float qmax = -INFINITY, hinge = 0.f;
    for (int k = 0; k < K; ++k) {
      const float raw = xs[(int64_t)k * a.T];
      const float s = fmaxf(raw, a.lsm);
      const float inv = expf(-s);
      const float c = y - xm[(int64_t)k * a.T];
      float L, gm, gs;
      if (low) {
        const float u = inv * ((c + a.h) + a.hl);
        const Sig su = sig_of(u);
        L = -su.sn;
        gm = -inv * su.neg;
        gs = -u * su.neg;
      } else if (high) {
        const float v = inv * ((c - a.h) - a.hl);
        const Sig sv = sig_of(v);
        L = -sv.sp;
        gm = inv * sv.pos;
        gs = v * sv.pos;
      } else {
        const float u = inv * ((c + a.h) + a.hl), v = inv * ((c - a.h) - a.hl);
        const float d = inv * a.h2;
        const Sig su = sig_of(u), sv = sig_of(v);
        const float E = -expm1f(-d);
        const float delta = su.pos * sv.neg * E;
        if (delta > 1e-5f) {
          // sg(u) - sg(-v): by the tails where y lies well inside the bin (both tanh near +-1 would cancel)
          const float half = su.th > 0.5f && sv.th < -0.5f ? sv.pos - su.neg : 0.5f * (su.th + sv.th);
          L = (-su.sn - sv.sp) + logf(E);
          gm = inv * half;
          gs = v * half - d * su.neg / (sv.neg * E);
        } else {
          const float m = inv * c;
          const Sig sm = sig_of(m);
          L = ((m - s) - 2.f * sm.sp) - a.log_half;
          gm = inv * sm.th;
          gs = m * sm.th - 1.f;
        }
      }
      if (a.hinge) hinge += fmaxf(0.f, -raw - a.log_nc);
      const float q = L + ((xl[(int64_t)k * a.T] - lmax) - llog);
      kq[(int64_t)k * THREADS] = q;
      km[(int64_t)k * THREADS] = gm;
      ks[(int64_t)k * THREADS] = raw >= a.lsm ? gs : 0.f;
      qmax = fmaxf(qmax, q);
    }
    float qsum = 0.f;
    for (int k = 0; k < K; ++k) qsum += expf(kq[(int64_t)k * THREADS] - qmax);
    l = wr * (hinge - (qmax + logf(qsum)));
    if (a.grad) {
      float* gl = a.grad + base;
      float* gmean = gl + (int64_t)K * a.T;
      float* gscale = gmean + (int64_t)K * a.T;
      const float rq = 1.f / qsum, rl = 1.f / lsum;
      for (int k = 0; k < K; ++k) {
        const int64_t o = (int64_t)k * a.T;
        const float p = expf(kq[(int64_t)k * THREADS] - qmax) * rq;
        const float sm = expf(xl[o] - lmax) * rl;
        float g = -p * ks[(int64_t)k * THREADS];
        if (a.hinge && -xs[o] - a.log_nc > 0.f) g -= 1.f;
        gl[o] = wr * (sm - p);
        gmean[o] = wr * (-p * km[(int64_t)k * THREADS]);
        gscale[o] = wr * g;
      }
    }
  } else if (a.grad && t < a.T) {
    float* gp = a.grad + base;
    for (int k = 0; k < 3 * K; ++k) gp[(int64_t)k * a.T] = 0.f;
  }
  if (have && a.elem) a.elem[r] = l;
  const double tot = block_sum((double)l, red);
  if (tid == 0) a.partial[b * gridDim.x + blockIdx.x] = tot;
}

template <int THREADS>
void launch_mol(const MolArgs& a, int B, hipStream_t s) {
  const size_t lds = (size_t)3 * a.K * THREADS * sizeof(float);
  mol_kernel<THREADS><<<dim3((unsigned)mol_chunks(a.T, THREADS), (unsigned)B), THREADS, lds, s>>>(a);
}

// ---- mu-law --------------------------------------------------------------------------------------------------
// (the index itself: mulaw_index, rawwave.h)
__global__ __launch_bounds__(RW_THREADS) void mulaw_encode_kernel(const double* __restrict__ x, int64_t n, double mu,
                                                                  double log1pmu, int64_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * RW_THREADS + threadIdx.x;
  if (i < n) idx[i] = mulaw_index(x[i], mu, log1pmu);
}

__global__ __launch_bounds__(RW_THREADS) void mulaw_decode_kernel(const int64_t* __restrict__ idx, int64_t n, double mu,
                                                                  double* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * RW_THREADS + threadIdx.x;
  if (i >= n) return;
  const double r = __dadd_rn(__ddiv_rn((double)idx[i], mu / 2.0), -1.0);
  const double sgn = (double)((r > 0.0) - (r < 0.0));
  y[i] = __dmul_rn(__ddiv_rn(sgn, mu), __dadd_rn(pow(1.0 + mu, fabs(r)), -1.0));
}

constexpr int OH_ROWS = 64;     // rows of a workgroup: their indices first, then the rows written lane-contiguously

struct OnehotArgs {
  const double* x;
  const int64_t* begin;         // [n_signals]: first sample of signal s in x
  const int64_t* out_off;       // [n_signals + 1]: rows of the output
  float* out;
  double mu, log1pmu;
  int W, sig0;                  // mu + 1
};

__global__ __launch_bounds__(RW_THREADS) void mulaw_onehot_kernel(OnehotArgs a) {
  __shared__ int64_t idx[OH_ROWS];
  const int sig = a.sig0 + blockIdx.y;
  const int64_t row0 = a.out_off[sig], n = a.out_off[sig + 1] - row0;
  const int64_t r0 = (int64_t)blockIdx.x * OH_ROWS;
  if (r0 >= n) return;
  const int rows = (int)min((int64_t)OH_ROWS, n - r0);
  if ((int)threadIdx.x < rows) idx[threadIdx.x] = mulaw_index(a.x[a.begin[sig] + r0 + threadIdx.x], a.mu, a.log1pmu);
  __syncthreads();
  float* out = a.out + (row0 + r0) * a.W;
  const int64_t total = (int64_t)rows * a.W;
  for (int64_t e = threadIdx.x; e < total; e += RW_THREADS) {
    const int rr = (int)(e / a.W);
    const int64_t c = e - (int64_t)rr * a.W;
    out[e] = c == idx[rr] ? 1.f : 0.f;
  }
}

// ---- sample_linearly -----------------------------------------------------------------------------------------
struct LinArgs {
  const void* x;
  void* y;
  const int64_t* off;           // [n_signals + 1] input rows; output rows are m times these
  int D, m, sig0;
};

// one element of the output a lane: row j = e / D of the signal's m T rows, column d (the arithmetic: lin_pos and
// lin_value, rawwave.h)
template <typename TI, typename TO>
__global__ __launch_bounds__(RW_THREADS) void sample_linearly_kernel(LinArgs a) {
  const int sig = a.sig0 + blockIdx.y;
  const int64_t begin = a.off[sig], T = a.off[sig + 1] - begin;
  const int64_t n_out = T * a.m;
  const int64_t e = (int64_t)blockIdx.x * RW_THREADS + threadIdx.x;
  if (e >= n_out * a.D) return;
  const int64_t j = e / a.D;
  const int d = (int)(e - j * a.D);
  const TI* x = reinterpret_cast<const TI*>(a.x) + begin * a.D + d;
  TO* y = reinterpret_cast<TO*>(a.y) + begin * a.m * a.D;
  y[e] = (TO)lin_value(x, a.D, lin_pos(j, T, n_out));
}

// offsets of a batch: ascending from 0; the longest signal
int rw_check_offsets(const char* func, const int64_t* h_off, int n_signals, int64_t* longest) {
  *longest = 0;
  for (int s = 0; s < n_signals; ++s) {
    const int64_t len = h_off[s + 1] - h_off[s];
    if (len < 0 || h_off[0] != 0) {
      set_error(std::string(func) + ": offsets must start at 0 and not decrease (signal " + std::to_string(s) + ")");
      return ITTS_E_INVALID;
    }
    *longest = std::max(*longest, len);
  }
  return ITTS_OK;
}

#define RW_REQUIRE_MU()                                                                                         \
  ITTS_REQUIRE(mu >= 1 && mu <= 65535, "mu = " + std::to_string(mu) + " is outside 1 .. 65535")
#define RW_REQUIRE_GRID(blocks, what)                                                                           \
  ITTS_REQUIRE((int64_t)(blocks) <= RW_MAX_GRID_X, std::to_string((int64_t)(blocks)) + " workgroups for " + (what) + \
                                                       ": more than " + std::to_string(RW_MAX_GRID_X))

}  // namespace
}  // namespace itts

using namespace itts;

extern "C" int64_t itts_mol_loss_workspace_bytes(int B, int64_t T) {
  if (B <= 0 || T <= 0) return 0;
  return B * mol_chunks(T, 64) * (int64_t)sizeof(double);       // (the smallest workgroup: the most partials)
}

extern "C" int itts_mol_loss(const float* d_x, const float* d_y, const float* d_w, int B, int K, int64_t T, int shift,
                             int num_classes, double log_scale_min, int hinge, float* d_loss, float* d_elem,
                             float* d_grad, void* d_workspace, void* stream) {
  ITTS_REQUIRE(K >= 1 && K <= MOL_MAX_K, "K = " + std::to_string(K) + " mixtures is outside 1 .. " +
                                             std::to_string(MOL_MAX_K));
  ITTS_REQUIRE(num_classes >= 2, "num_classes = " + std::to_string(num_classes) + " is below 2");
  ITTS_REQUIRE(B >= 0, "B = " + std::to_string(B) + " is negative");
  ITTS_REQUIRE(B <= 65535, "B = " + std::to_string(B) + " exceeds 65535");
  ITTS_REQUIRE(T >= 1, "T = " + std::to_string(T) + " is not positive");
  ITTS_REQUIRE(shift >= 0 && shift < T,
               "shift = " + std::to_string(shift) + " is outside 0 .. T - 1 = " + std::to_string(T - 1));
  ITTS_REQUIRE(mol_chunks(T, 64) <= 0x7fffffff, "T = " + std::to_string(T) + " is too large");
  ITTS_REQUIRE(log_scale_min == log_scale_min, "log_scale_min is not a number");
  ITTS_REQUIRE(d_loss, "null pointer (d_loss)");
  hipStream_t s = as_stream(stream);
  if (B == 0) {
    ITTS_HIP_CHECK(hipMemsetAsync(d_loss, 0, sizeof(float), s));
    return ITTS_OK;
  }
  ITTS_REQUIRE(d_x && d_y && d_w && d_workspace,
               "null pointer (d_x / d_y / d_w / d_workspace) with B = " + std::to_string(B));
  MolArgs a{};
  a.x = d_x; a.y = d_y; a.w = d_w; a.elem = d_elem; a.grad = d_grad;
  a.partial = reinterpret_cast<double*>(d_workspace);
  a.T = T; a.Tn = T - shift; a.K = K; a.shift = shift; a.hinge = hinge != 0;
  a.h = (float)(1.0 / (num_classes - 1));
  a.hl = (float)(1.0 / (num_classes - 1) - (double)a.h);
  a.h2 = 2.f * a.h;
  a.lsm = (float)log_scale_min;
  a.log_nc = (float)log((double)num_classes);
  a.log_half = (float)log((num_classes - 1) / 2.0);
  const int threads = mol_threads(K);
  if (threads == 256) launch_mol<256>(a, B, s);
  else if (threads == 128) launch_mol<128>(a, B, s);
  else launch_mol<64>(a, B, s);
  ITTS_LAUNCH_CHECK();
  return loss_final_sum(a.partial, mol_chunks(T, threads) * B, 1.0, d_loss, s);
}

extern "C" int itts_mulaw_encode_f64(const double* d_x, const int64_t* h_offsets, int n_signals, int mu,
                                     int64_t* d_index, void* stream) {
  RW_REQUIRE_MU();
  ITTS_REQUIRE(n_signals >= 0, "n_signals = " + std::to_string(n_signals) + " is negative");
  if (n_signals == 0) return ITTS_OK;
  ITTS_REQUIRE(h_offsets, "null pointer: h_offsets");
  int64_t longest = 0;
  if (int rc = rw_check_offsets(__func__, h_offsets, n_signals, &longest)) return rc;
  const int64_t n = h_offsets[n_signals];
  if (n == 0) return ITTS_OK;
  const int64_t blocks = (n + RW_THREADS - 1) / RW_THREADS;
  RW_REQUIRE_GRID(blocks, "the batch");
  ITTS_REQUIRE(d_x && d_index, "null pointer with n_signals = " + std::to_string(n_signals));
  mulaw_encode_kernel<<<dim3((unsigned)blocks), RW_THREADS, 0, as_stream(stream)>>>(d_x, n, (double)mu,
                                                                                   log(1.0 + mu), d_index);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_mulaw_decode(const int64_t* d_index, const int64_t* h_offsets, int n_signals, int mu, double* d_y,
                                 void* stream) {
  RW_REQUIRE_MU();
  ITTS_REQUIRE(n_signals >= 0, "n_signals = " + std::to_string(n_signals) + " is negative");
  if (n_signals == 0) return ITTS_OK;
  ITTS_REQUIRE(h_offsets, "null pointer: h_offsets");
  int64_t longest = 0;
  if (int rc = rw_check_offsets(__func__, h_offsets, n_signals, &longest)) return rc;
  const int64_t n = h_offsets[n_signals];
  if (n == 0) return ITTS_OK;
  const int64_t blocks = (n + RW_THREADS - 1) / RW_THREADS;
  RW_REQUIRE_GRID(blocks, "the batch");
  ITTS_REQUIRE(d_index && d_y, "null pointer with n_signals = " + std::to_string(n_signals));
  mulaw_decode_kernel<<<dim3((unsigned)blocks), RW_THREADS, 0, as_stream(stream)>>>(d_index, n, (double)mu, d_y);
  ITTS_LAUNCH_CHECK();
  return ITTS_OK;
}

extern "C" int itts_mulaw_onehot(const double* d_x, const int64_t* h_begin, const int64_t* h_out_offsets,
                                 int n_signals, int mu, float* d_onehot, void* stream) {
  RW_REQUIRE_MU();
  ITTS_REQUIRE(n_signals >= 0, "n_signals = " + std::to_string(n_signals) + " is negative");
  if (n_signals == 0) return ITTS_OK;
  ITTS_REQUIRE(h_begin && h_out_offsets, "null pointer: offsets");
  int64_t longest = 0;
  if (int rc = rw_check_offsets(__func__, h_out_offsets, n_signals, &longest)) return rc;
  for (int s = 0; s < n_signals; ++s)
    ITTS_REQUIRE(h_begin[s] >= 0, "signal " + std::to_string(s) + " begins at " + std::to_string(h_begin[s]));
  if (longest == 0) return ITTS_OK;
  RW_REQUIRE_GRID((longest + OH_ROWS - 1) / OH_ROWS, "the longest signal");
  ITTS_REQUIRE(d_x && d_onehot, "null pointer with n_signals = " + std::to_string(n_signals));
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  std::vector<int64_t> h((size_t)2 * n_signals + 1);
  std::copy(h_begin, h_begin + n_signals, h.begin());
  std::copy(h_out_offsets, h_out_offsets + n_signals + 1, h.begin() + n_signals);
  int64_t* d_off = nullptr;
  if (int rc = upload_i64(h.data(), (int)h.size(), &d_off, scratch)) return rc;
  OnehotArgs a{};
  a.x = d_x; a.begin = d_off; a.out_off = d_off + n_signals; a.out = d_onehot;
  a.mu = (double)mu; a.log1pmu = log(1.0 + mu); a.W = mu + 1;
  for (int s0 = 0; s0 < n_signals; s0 += RW_MAX_GRID_Y) {
    a.sig0 = s0;
    const unsigned ny = (unsigned)std::min(RW_MAX_GRID_Y, n_signals - s0);
    mulaw_onehot_kernel<<<dim3((unsigned)((longest + OH_ROWS - 1) / OH_ROWS), ny), RW_THREADS, 0, s>>>(a);
    ITTS_LAUNCH_CHECK();
  }
  return ITTS_OK;
}

extern "C" int itts_sample_linearly(const void* d_x, int in_f64, const int64_t* h_offsets, int n_signals, int D, int m,
                                    void* d_y, int out_f64, void* stream) {
  ITTS_REQUIRE(m >= 1, "in_to_out_multiplier m = " + std::to_string(m) + " is below 1");
  ITTS_REQUIRE(D >= 1, "D = " + std::to_string(D) + " is not positive");
  ITTS_REQUIRE(n_signals >= 0, "n_signals = " + std::to_string(n_signals) + " is negative");
  if (n_signals == 0) return ITTS_OK;
  ITTS_REQUIRE(h_offsets, "null pointer: h_offsets");
  int64_t longest = 0;
  if (int rc = rw_check_offsets(__func__, h_offsets, n_signals, &longest)) return rc;
  for (int s = 0; s < n_signals; ++s) {
    const int64_t len = h_offsets[s + 1] - h_offsets[s];
    ITTS_REQUIRE(len >= 2, "signal " + std::to_string(s) + " has " + std::to_string(len) +
                               " frames: linear interpolation needs at least 2");
  }
  const int64_t blocks = (longest * m * D + RW_THREADS - 1) / RW_THREADS;
  RW_REQUIRE_GRID(blocks, "the longest signal");
  ITTS_REQUIRE(d_x && d_y, "null pointer with n_signals = " + std::to_string(n_signals));
  hipStream_t s = as_stream(stream);
  ScratchScope scratch(s);
  int64_t* d_off = nullptr;
  if (int rc = upload_i64(h_offsets, n_signals + 1, &d_off, scratch)) return rc;
  LinArgs a{};
  a.x = d_x; a.y = d_y; a.off = d_off; a.D = D; a.m = m;
  for (int s0 = 0; s0 < n_signals; s0 += RW_MAX_GRID_Y) {
    a.sig0 = s0;
    const dim3 grid((unsigned)blocks, (unsigned)std::min(RW_MAX_GRID_Y, n_signals - s0));
    if (in_f64 && out_f64) sample_linearly_kernel<double, double><<<grid, RW_THREADS, 0, s>>>(a);
    else if (in_f64) sample_linearly_kernel<double, float><<<grid, RW_THREADS, 0, s>>>(a);
    else if (out_f64) sample_linearly_kernel<float, double><<<grid, RW_THREADS, 0, s>>>(a);
    else sample_linearly_kernel<float, float><<<grid, RW_THREADS, 0, s>>>(a);
    ITTS_LAUNCH_CHECK();
  }
  return ITTS_OK;
}
