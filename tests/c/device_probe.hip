// device_probe.hip -- test-only probes of the sampler's device primitives.
//
// Elementwise, bounds-checked kernels that call the product's own device functions
// (olpe_device.h, exp_table.h) on caller arrays, and a one-wave kernel that reports the
// FAST guards' verdict for a parameter vector.  Loaded with ctypes by
// tests/test_gpu_device_math.py and tests/test_gpu_fast_guards.py; built by
// olpefit_amd/build.py (build_probe) with the product's flags into
// olpefit_amd/libolpe_probe.so.  Every entry point takes host pointers, returns a HIP
// status (0 = hipSuccess) and never aborts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "olpe_device.h"

using namespace olpe;

namespace {

enum Op {
  OP_EXPTAB = 0,      // in x            -> out ExpTab::operator()(x)
  OP_EXPTAB_RAW = 1,  // in x            -> out ExpTab::raw(x)      (x within [-1000, 710])
  OP_EXP_NEG = 2,     // in q            -> out exp_neg(q), ocml exp(-q)
  OP_SINCOS = 3,      // in th           -> out sin, cos            (|th| <= pi/4)
  OP_TRIG_FAST = 4,   // in th           -> out cos^2, sin^2, sin 2th  (make_trig<true>)
  OP_TRIG_EXACT = 5,  //                                               (make_trig<false>)
  OP_COEF_FAST = 6,   // in sx, sy, th   -> out a, b, c  (make_coef<true> o make_trig<true>)
  OP_COEF_EXACT = 7,  //                                 (make_coef<false> o make_trig<false>)
  OP_THRESHOLD = 8,   // in u            -> out accept_threshold(u)
  OP_COUNT
};

__host__ __device__ constexpr int op_nin(int op) { return op == OP_COEF_FAST || op == OP_COEF_EXACT ? 3 : 1; }
__host__ __device__ constexpr int op_nout(int op) {
  return op == OP_EXP_NEG || op == OP_SINCOS ? 2
         : (op >= OP_TRIG_FAST && op <= OP_COEF_EXACT) ? 3 : 1;
}

// in[k * n + i] = input k of element i, out[k * n + i] = output k
__global__ __launch_bounds__(256) void probe_kernel(int op, const double *in, long long n,
                                                    double *out) {
  __shared__ double etab[64];
  // the samplers' LDS copy of the 2^(j/64) table
  if (threadIdx.x < 64) etab[threadIdx.x] = c_exp2_64[threadIdx.x];
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ExpTab ex{etab};
  const double x = in[i];
  switch (op) {
    case OP_EXPTAB: out[i] = ex(x); break;
    case OP_EXPTAB_RAW: out[i] = ex.raw(x); break;
    case OP_EXP_NEG:
      out[i] = exp_neg(x);
      out[n + i] = exp(-x);
      break;
    case OP_SINCOS: {
      double s, c;
      sincos_small(x, &s, &c);
      out[i] = s;
      out[n + i] = c;
      break;
    }
    case OP_TRIG_FAST:
    case OP_TRIG_EXACT: {
      const Trig t = op == OP_TRIG_FAST ? make_trig<true>(x) : make_trig<false>(x);
      out[i] = t.cost2;
      out[n + i] = t.sint2;
      out[2 * n + i] = t.sin2t;
      break;
    }
    case OP_COEF_FAST:
    case OP_COEF_EXACT: {
      const double sy = in[n + i], th = in[2 * n + i];
      const Coef k = op == OP_COEF_FAST ? make_coef<true>(x, sy, make_trig<true>(th))
                                        : make_coef<false>(x, sy, make_trig<false>(th));
      out[i] = k.a;
      out[n + i] = k.b;
      out[2 * n + i] = k.c;
      break;
    }
    case OP_THRESHOLD: out[i] = accept_threshold(x); break;
    default: break;
  }
}

// One wave per parameter vector: the FAST model descriptor of olpe_eval_kernel
// (make_trig<true>, make_coef<true>, make_model), placed in LDS as the samplers keep it,
// then the guards with the row count and reference step of sweep<>.
// out[4 w + 0] = fast3_fails, [1] = fast3_cols_pass over those, [2] = fast3_amp_ok over
// those, [3] = fast_level.
template <int NSRC>
__global__ __launch_bounds__(64) void guard_kernel(const double *params, int W, int n,
                                                   int bkgd_mode, uint32_t *out) {
  using L = Layout<NSRC>;
  constexpr int PS = L::PS;
  __shared__ ModelDesc<NSRC> md;
  const int lane = threadIdx.x;
  const int w = blockIdx.x;
  if (w >= W) return;
  double p[PS];
#pragma unroll
  for (int k = 0; k < PS; ++k) p[k] = uniform_f64(params[(size_t)w * PS + k]);
  auto q = [&](int k) -> double { return p[k]; };
  const Trig T1 = make_trig<true>(p[L::T1]), T2 = make_trig<true>(p[L::T2]);
  const ModelDesc<NSRC> m = make_model<NSRC>(
      q, make_coef<true>(p[L::S1X], p[L::S1Y], T1), make_coef<true>(p[L::S2X], p[L::S2Y], T2),
      bkgd_mode);
  if (lane == 0) md = m;
  __syncthreads();
  const int S = row_stride(n);
  const int rows0 = (n + S - 1) / S;
  const int kc = rows0 / 2;
  const unsigned fails = fast3_fails<NSRC>(md, n, rows0, kc, lane);
  const unsigned pass = fails ? fast3_cols_pass<NSRC>(md, n, rows0, kc, lane, fails) : 0u;
  const bool amp = fast3_amp_ok<NSRC>(md, lane, fails);
  const int lvl = fast_level<NSRC>(md, n);
  if (lane == 0) {
    out[4 * w + 0] = fails;
    out[4 * w + 1] = pass;
    out[4 * w + 2] = amp ? 1u : 0u;
    out[4 * w + 3] = (uint32_t)lvl;
  }
}

struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace

extern "C" {

// number of input / output arrays of an op (-1: no such op)
int olpe_probe_nin(int op) { return op >= 0 && op < OP_COUNT ? op_nin(op) : -1; }
int olpe_probe_nout(int op) { return op >= 0 && op < OP_COUNT ? op_nout(op) : -1; }

// in: op_nin(op) arrays of n doubles, one after the other; out: op_nout(op) arrays
int olpe_probe_run(int op, const double *in, long long n, double *out) {
  if (op < 0 || op >= OP_COUNT || n <= 0 || n > (1ll << 26) || !in || !out)
    return (int)hipErrorInvalidValue;
  const size_t bi = (size_t)op_nin(op) * n * sizeof(double);
  const size_t bo = (size_t)op_nout(op) * n * sizeof(double);
  DevBuf di, dout;
  hipError_t e;
  if ((e = hipMalloc(&di.p, bi)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&dout.p, bo)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(di.p, in, bi, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemset(dout.p, 0, bo)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op,
                     (const double *)di.p, n, (double *)dout.p);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  return (int)hipMemcpy(out, dout.p, bo, hipMemcpyDeviceToHost);
}

// params: W vectors of PS doubles (17 for nsrc 2, 20 for nsrc 3; the last is chi^2 and is
// not read); out: 4 words per vector (guard_kernel)
int olpe_probe_guards(int nsrc, int n, int bkgd_mode, const double *params, int W,
                      uint32_t *out) {
  if ((nsrc != 2 && nsrc != 3) || n < 2 || n > 4096 || W <= 0 || W > (1 << 20) || !params ||
      !out)
    return (int)hipErrorInvalidValue;
  const size_t ps = nsrc == 2 ? Layout<2>::PS : Layout<3>::PS;
  const size_t bi = ps * (size_t)W * sizeof(double), bo = 4 * (size_t)W * sizeof(uint32_t);
  DevBuf di, dout;
  hipError_t e;
  if ((e = hipMalloc(&di.p, bi)) != hipSuccess) return (int)e;
  if ((e = hipMalloc(&dout.p, bo)) != hipSuccess) return (int)e;
  if ((e = hipMemcpy(di.p, params, bi, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
  if ((e = hipMemset(dout.p, 0, bo)) != hipSuccess) return (int)e;
  if (nsrc == 2)
    hipLaunchKernelGGL(guard_kernel<2>, dim3((unsigned)W), dim3(64), 0, 0,
                       (const double *)di.p, W, n, bkgd_mode, (uint32_t *)dout.p);
  else
    hipLaunchKernelGGL(guard_kernel<3>, dim3((unsigned)W), dim3(64), 0, 0,
                       (const double *)di.p, W, n, bkgd_mode, (uint32_t *)dout.p);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
  return (int)hipMemcpy(out, dout.p, bo, hipMemcpyDeviceToHost);
}

}  // extern "C"
