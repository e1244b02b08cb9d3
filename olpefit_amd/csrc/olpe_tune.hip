// olpe_tune.hip -- the sampler's jump widths as a per-context run-time quantity
// (olpe_widths_set / olpe_widths_get) and the acceptance-rate tuner that adapts them on
// the device between launches (olpe_tune_*; include/olpe.h states the rule).
//
// The widths a launch reads are olpe_ctx::d_widths (olpe.hip, width_of).  Everything here
// that changes them is a small launch on the context's stream, so it is ordered with the
// sampler launches around it and the host never waits:
//   widths_set_kernel   the widths of olpe_widths_set, carried in the kernel's arguments
//                       (no host buffer has to outlive the call)
//   tune_sum_kernel     the 64-bit sums over walkers of tries[.][j] and accepts[.][j]: a
//                       capped grid, a thread adding the walkers t, t + threads, ... in
//                       registers, the block tree of olpe_reduce.h per column, one integer
//                       atomic add per block and column -- integer sums, exact in any order
//   tune_update_kernel  one thread per parameter: the deltas against the previous sums,
//                       the rule, the log record
// Nothing writes d_widths while a sampler launch runs: the stream orders them.
#include <hip/hip_runtime.h>

#include <math.h>

#include <algorithm>
#include <vector>

#include "../../include/olpe.h"
#include "olpe_internal.h"
#include "olpe_reduce.h"

using namespace olpe;

namespace {

constexpr int kP = 19;                   // columns reserved per array (P = 16 or 19)
constexpr int kThreads = 256;
constexpr int kMaxBlocks = 64;           // grid cap of tune_sum_kernel
constexpr int kTuneLog = OLPE_TUNE_LOG;  // steps the device log holds

struct TuneRec {
  long long dT[kP], dA[kP];
  double w[kP];
};
// d_tune: the sums of this step, the sums of the step before, the log
struct TuneBuf {
  unsigned long long now[2 * kP];
  long long prev[2 * kP];
  TuneRec log[kTuneLog];
};

struct WidthsArg {
  double w[kP];
};

__global__ void widths_set_kernel(int np, WidthsArg a, double *w) {
  const int j = threadIdx.x;
  if (j < np) w[j] = a.w[j];
}

template <int NP>
__global__ __launch_bounds__(kThreads) void tune_sum_kernel(const uint32_t *__restrict__ tries,
                                                            const uint32_t *__restrict__ acc,
                                                            long long W, unsigned long long *now) {
  __shared__ unsigned long long red[kThreads];
  unsigned long long t[NP], a[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) t[j] = a[j] = 0ull;
  const long long step = (long long)gridDim.x * kThreads;
  for (long long w = (long long)blockIdx.x * kThreads + threadIdx.x; w < W; w += step) {
    const uint32_t *tr = tries + (size_t)w * NP, *ac = acc + (size_t)w * NP;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      t[j] += tr[j];
      a[j] += ac[j];
    }
  }
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const unsigned long long st = block_word<kThreads, WordSum>(t[j], red);
    const unsigned long long sa = block_word<kThreads, WordSum>(a[j], red);
    if (threadIdx.x == 0) {
      atomicAdd(now + j, st);
      atomicAdd(now + kP + j, sa);
    }
  }
}

// rec == null: the baseline of olpe_tune_begin (the sums become the previous ones).
// Otherwise step k's update, g = gain / sqrt(k) from the host: every operation below is one
// IEEE double operation in the order include/olpe.h states (the library is built without
// contraction), so a NumPy restatement gives the same bits.
__global__ void tune_update_kernel(int np, TuneBuf *b, double *w, const double *wdef, double g,
                                   double target, TuneRec *rec) {
  const int j = threadIdx.x;
  if (j >= np) return;
  const long long T = (long long)b->now[j], A = (long long)b->now[kP + j];
  if (rec) {
    const long long dT = T - b->prev[j], dA = A - b->prev[kP + j];
    double wj = w[j];
    if (dT > 0) {
      const double a = (double)dA / (double)dT;
      const double f = 1.0 + g * (a - target);
      double v = wj * f;
      const double lo = wdef[j] / 1024.0, hi = wdef[j] * 64.0;
      v = v < lo ? lo : v;
      v = v > hi ? hi : v;
      wj = v;
      w[j] = wj;
    }
    rec->dT[j] = dT;
    rec->dA[j] = dA;
    rec->w[j] = wj;
  }
  b->prev[j] = T;
  b->prev[kP + j] = A;
}

// the sums of the counters as they are when the stream gets here, into b->now
int enqueue_sums(olpe_ctx *c, TuneBuf *b) {
  HIPCHK(hipMemsetAsync(b->now, 0, sizeof(b->now), olpe_main(c)));
  const unsigned blocks =
      (unsigned)std::min<long long>(((long long)c->W + kThreads - 1) / kThreads, kMaxBlocks);
  if (c->np == 16)
    hipLaunchKernelGGL(tune_sum_kernel<16>, dim3(blocks), dim3(kThreads), 0, olpe_main(c), c->d_tries,
                       c->d_acc, (long long)c->W, b->now);
  else
    hipLaunchKernelGGL(tune_sum_kernel<19>, dim3(blocks), dim3(kThreads), 0, olpe_main(c), c->d_tries,
                       c->d_acc, (long long)c->W, b->now);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_widths_set(olpe_ctx *c, const double *w) {
  if (!c) return set_err(OLPE_EINVAL, "NULL ctx");
  HIPCHK(hipSetDevice(c->device));
  if (!w) return olpe_widths_defaults(c, false);
  for (int j = 0; j < c->np; ++j) {
    if (!std::isfinite(w[j]) || !(w[j] > 0.0))
      return set_err(OLPE_EINVAL, "width %d is %g: widths are finite and > 0", j, w[j]);
    if (((c->logmask >> j) & 1u) && w[j] > OLPE_LOG_WIDTH_MAX)
      return set_err(OLPE_EINVAL, "width %d is %g dex: a log-proposed parameter takes at most %g",
                     j, w[j], (double)OLPE_LOG_WIDTH_MAX);
  }
  WidthsArg a = {};
  for (int j = 0; j < c->np; ++j) a.w[j] = w[j];
  hipLaunchKernelGGL(widths_set_kernel, dim3(1), dim3(64), 0, olpe_main(c), c->np, a, c->d_widths);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

int olpe_widths_get(olpe_ctx *c, double *out) {
  if (!c || !out) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out, c->d_widths, (size_t)c->np * 8, hipMemcpyDeviceToHost, olpe_main(c)));
  HIPCHK(hipStreamSynchronize(olpe_main(c)));
  return OLPE_OK;
}

int olpe_tune_begin(olpe_ctx *c, double target, double gain) {
  if (!c) return set_err(OLPE_EINVAL, "NULL ctx");
  if (!(target > 0.0 && target < 1.0) || !(gain > 0.0) || !std::isfinite(gain) ||
      !(gain * target < 1.0))
    return set_err(OLPE_EINVAL, "tuner: 0 < target < 1, gain > 0 and gain * target < 1 "
                   "(got target %g, gain %g)", target, gain);
  if (!c->d_tries || !c->d_acc) return set_err(OLPE_ESTATE, "call olpe_seed first");
  HIPCHK(hipSetDevice(c->device));
  if (!c->d_tune) {
    if (hipMalloc(&c->d_tune, sizeof(TuneBuf)) != hipSuccess) {
      c->d_tune = nullptr;
      (void)hipGetLastError();
      return set_err(OLPE_ENOMEM, "hipMalloc(%zu bytes) for the tuner", sizeof(TuneBuf));
    }
  }
  TuneBuf *b = static_cast<TuneBuf *>(c->d_tune);
  c->tune_on = false;
  int rc;
  if ((rc = enqueue_sums(c, b))) return rc;
  hipLaunchKernelGGL(tune_update_kernel, dim3(1), dim3(64), 0, olpe_main(c), c->np, b, c->d_widths,
                     c->d_wdef, 0.0, target, (TuneRec *)nullptr);
  HIPCHK(hipGetLastError());
  c->tune_on = true;
  c->tune_k = 0;
  c->tune_target = target;
  c->tune_gain = gain;
  return OLPE_OK;
}

int olpe_tune_step(olpe_ctx *c) {
  if (!c) return set_err(OLPE_EINVAL, "NULL ctx");
  if (!c->tune_on) return set_err(OLPE_ESTATE, "call olpe_tune_begin first");
  if (c->tune_k >= kTuneLog)
    return set_err(OLPE_ESTATE, "the tuner's log holds %d steps: end the session", kTuneLog);
  if (!c->d_tries || !c->d_acc) return set_err(OLPE_ESTATE, "no ensemble");
  HIPCHK(hipSetDevice(c->device));
  TuneBuf *b = static_cast<TuneBuf *>(c->d_tune);
  int rc;
  if ((rc = enqueue_sums(c, b))) return rc;
  const int k = c->tune_k + 1;
  const double g = c->tune_gain / sqrt((double)k);
  hipLaunchKernelGGL(tune_update_kernel, dim3(1), dim3(64), 0, olpe_main(c), c->np, b, c->d_widths,
                     c->d_wdef, g, c->tune_target, b->log + (k - 1));
  HIPCHK(hipGetLastError());
  c->tune_k = k;
  return OLPE_OK;
}

int olpe_tune_get(olpe_ctx *c, int *steps, long long *dT, long long *dA, double *widths) {
  if (!c || !steps) return set_err(OLPE_EINVAL, "NULL argument");
  if (!c->d_tune) return set_err(OLPE_ESTATE, "no tuning session yet");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(olpe_main(c)));
  const int k = c->tune_k;
  *steps = k;
  if (!k || (!dT && !dA && !widths)) return OLPE_OK;
  std::vector<TuneRec> h((size_t)k);
  HIPCHK(hipMemcpy(h.data(), static_cast<TuneBuf *>(c->d_tune)->log, (size_t)k * sizeof(TuneRec),
                   hipMemcpyDeviceToHost));
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < c->np; ++j) {
      if (dT) dT[(size_t)i * c->np + j] = h[i].dT[j];
      if (dA) dA[(size_t)i * c->np + j] = h[i].dA[j];
      if (widths) widths[(size_t)i * c->np + j] = h[i].w[j];
    }
  return OLPE_OK;
}

int olpe_tune_end(olpe_ctx *c) {
  if (!c) return set_err(OLPE_EINVAL, "NULL ctx");
  if (!c->tune_on) return set_err(OLPE_ESTATE, "no tuning session to end");
  c->tune_on = false;
  return OLPE_OK;
}

}  // extern "C"
