// olpe_normal.hip -- the Gauss-Newton normal equations of the model at explicit parameter
// vectors: chi^2 = sum r^2, g = J^T r and J^T J over the context's cutout, with
// r_p = (D_p - M_p) / err_p and J_pk = (dM_p / dtheta_k) / err_p.  The reference has no
// optimiser; the model is build_analytical_model (apf_step2.py:106-124; 3body :106-125) in
// the EXACT operation order (make_desc / pixel_model of olpe_samples.h), whatever the
// context's eval mode, and the residual is chi_squared's (:134-137).  Everything after these
// sums (Levenberg-Marquardt, the Laplace approximation) is host algebra: olpefit_amd/mapfit.py.
//
// One wave per vector, kWaves vectors per workgroup, nothing shared between the waves.  A
// wave walks the cutout 64 pixels at a time, a pixel per lane (pixel 64 t + lane; lanes past
// the last pixel and masked pixels, staged {0, 0}, carry exact zeros).  Per pixel a lane forms
// the 2 NSRC exponentials once, from them the derivatives with respect to each Gaussian's
// {amp, x0, y0, a, b, c}, and through the wave-uniform chain rule of Chain the P columns
// J_pk.  chi^2 and g stay per-lane accumulators in this layout and go through the fixed-order
// wave_sum at the end.  The P x P sum goes to the matrix core: the lane writes its row of
// weighted derivatives into a wave-private LDS tile [64 pixels][S] (S odd: the rows fall on
// distinct banks), and lane l reads back tile[4 m + (l >> 4)][l & 15], m = 0 .. 15, which is
// at once operand A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15] of
// v_mfma_f64_16x16x4_f64: sixteen MFMAs with the same register for A and B add the 64 pixels'
// outer products to a 16 x 16 tile held in 8 registers (C/D: column lane & 15, row
// (lane >> 4) + 4 reg).  With three sources columns 16 .. 18 ride in the same LDS rows: a
// second MFMA per step (A the low columns, B the three high ones, zero-padded to 16) gives
// the 16 x 3 block, and the 3 x 3 corner is six per-lane accumulators beside g (a third MFMA
// instead was measured and is slower: OLPE_NORMAL_CORNER).  The upper
// triangle is written to both halves, so jtj is symmetric to the bit.
//
// No atomics and no cross-wave combine: a vector's outputs take the same operations in the
// same order wherever it sits in the batch.  A non-finite parameter, or a model that is not
// finite at a usable pixel, makes that vector's outputs NaN.  DESIGN.md §7k.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/olpe.h"
#include "../../include/olpe_test.h"
#include "olpe_fold.h"
#include "olpe_internal.h"

// The sampler's device functions, by #include only (see olpe_resid.hip).
namespace olpe_normal_dev {
#include "olpe_device.h"
}
namespace dev = olpe_normal_dev::olpe;

using namespace olpe;

// make_desc and the per-pixel model's operation order, shared with the per-pixel folds
#include "olpe_samples.h"

namespace {

constexpr int kWaves = 4;                      // vectors per workgroup
typedef double v4d __attribute__((ext_vector_type(4)));

// The wave-uniform part of the chain rule from the Gaussians' {amp, x0, y0, a, b, c} to the
// P parameters: amplitudes through tot = A_s - off, wide = tot ratio, narrow = tot - wide;
// s1 (narrow set) and s2 (wide set): s[q][m] = d(a, b, c)[m] / d(sigma_x, sigma_y, theta)[q]
template <int NSRC> struct Chain {
  double ratio, nratio;
  double tot[NSRC];
  double s1[3][3], s2[3][3];
};

// a = (cos^2 / sx^2 + sin^2 / sy^2) / 2, b = sin 2t (1 / sx^2 - 1 / sy^2) / 2,
// c = (sin^2 / sx^2 + cos^2 / sy^2) / 2 (make_coef); at sx = sy the theta row is exactly 0
__device__ __forceinline__ void shape_jac(double sx, double sy, const dev::Trig &t,
                                          double (&s)[3][3]) {
  const double ix = 1.0 / (sx * sx), iy = 1.0 / (sy * sy);
  const double ix3 = ix / sx, iy3 = iy / sy;
  const double dxy = ix - iy, c2t = t.cost2 - t.sint2;
  s[0][0] = -(t.cost2 * ix3);
  s[0][1] = -(t.sin2t * ix3);
  s[0][2] = -(t.sint2 * ix3);
  s[1][0] = -(t.sint2 * iy3);
  s[1][1] = t.sin2t * iy3;
  s[1][2] = -(t.cost2 * iy3);
  s[2][0] = -0.5 * (t.sin2t * dxy);
  s[2][1] = c2t * dxy;
  s[2][2] = 0.5 * (t.sin2t * dxy);
}

template <int NSRC>
__device__ __forceinline__ Chain<NSRC> make_chain(const double *p) {
  using L = dev::Layout<NSRC>;
  Chain<NSRC> ch;
  ch.ratio = p[L::RATIO];
  ch.nratio = 1.0 - p[L::RATIO];
#pragma unroll
  for (int s = 0; s < NSRC; ++s) ch.tot[s] = p[L::sa(s)] - p[L::OFF];
  shape_jac(p[L::S1X], p[L::S1Y], dev::make_trig<false>(p[L::T1]), ch.s1);
  shape_jac(p[L::S2X], p[L::S2Y], dev::make_trig<false>(p[L::T2]), ch.s2);
  return ch;
}

// Pixel (column xj, row yi) of the model d (pixel_model's operations: the same bits) and
// its derivatives J[k] = dM / dtheta_k, unweighted
template <int NSRC>
__device__ __forceinline__ double pixel_jac(const double *d, const Chain<NSRC> &ch,
                                            int bkgd_mode, double xj, double yi, double *J) {
  using L = dev::Layout<NSRC>;
  constexpr int G = 2 * NSRC;
  double E[G], v[G], gx[G], gy[G], ga[G], gb[G], gc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const double a = d[6 * g + 3], b = d[6 * g + 4], c = d[6 * g + 5];
    const double xd = xj - d[6 * g + 1];
    const double t1 = a * (xd * xd);
    const double t2 = b * xd;
    const double yd = yi - d[6 * g + 2];
    const double qq = (t1 + t2 * yd) + c * (yd * yd);
    E[g] = dev::exp_neg(qq);
    v[g] = d[6 * g] * E[g];
    gx[g] = v[g] * ((2.0 * a) * xd + b * yd);
    gy[g] = v[g] * (t2 + (2.0 * c) * yd);
    ga[g] = -(v[g] * (xd * xd));
    gb[g] = -(v[g] * (xd * yd));
    gc[g] = -(v[g] * (yd * yd));
  }
  double mod = v[0] + v[1];
#pragma unroll
  for (int s = 1; s < NSRC; ++s) mod = mod + (v[2 * s] + v[2 * s + 1]);
  mod = mod + d[6 * G];
  // wide = Gaussian 2 s (set 2, centre moved by dx, dy), narrow = 2 s + 1 (set 1)
  double jdx = 0.0, jdy = 0.0, jr = 0.0, joff = 0.0;
  double n1[3] = {0.0, 0.0, 0.0}, n2[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int s = 0; s < NSRC; ++s) {
    J[L::sx(s)] = gx[2 * s] + gx[2 * s + 1];
    J[L::sy(s)] = gy[2 * s] + gy[2 * s + 1];
    jdx += gx[2 * s];
    jdy += gy[2 * s];
    const double ea = ch.ratio * E[2 * s] + ch.nratio * E[2 * s + 1];
    J[L::sa(s)] = ea;
    joff -= ea;
    jr += ch.tot[s] * (E[2 * s] - E[2 * s + 1]);
    n1[0] += ga[2 * s + 1];
    n1[1] += gb[2 * s + 1];
    n1[2] += gc[2 * s + 1];
    n2[0] += ga[2 * s];
    n2[1] += gb[2 * s];
    n2[2] += gc[2 * s];
  }
  J[L::DX] = jdx;
  J[L::DY] = jdy;
  J[L::RATIO] = jr;
  J[L::OFF] = joff;
  J[L::S1X] = (n1[0] * ch.s1[0][0] + n1[1] * ch.s1[0][1]) + n1[2] * ch.s1[0][2];
  J[L::S1Y] = (n1[0] * ch.s1[1][0] + n1[1] * ch.s1[1][1]) + n1[2] * ch.s1[1][2];
  J[L::T1] = (n1[0] * ch.s1[2][0] + n1[1] * ch.s1[2][1]) + n1[2] * ch.s1[2][2];
  J[L::S2X] = (n2[0] * ch.s2[0][0] + n2[1] * ch.s2[0][1]) + n2[2] * ch.s2[0][2];
  J[L::S2Y] = (n2[0] * ch.s2[1][0] + n2[1] * ch.s2[1][1]) + n2[2] * ch.s2[1][2];
  J[L::T2] = (n2[0] * ch.s2[2][0] + n2[1] * ch.s2[2][1]) + n2[2] * ch.s2[2][2];
  // the background's parameter (make_model): p[12] doubles as sigma_x of the wide set in
  // bkgd_mode 0 of the 2-source layout, as `off` with three sources
  J[L::BG_QUIRK] += bkgd_mode == 0 ? 1.0 : 0.0;
  J[L::BG_FIXED] += bkgd_mode == 0 ? 0.0 : 1.0;
  return mod;
}

template <int NSRC> constexpr int tile_stride() { return NSRC == 2 ? 17 : 21; }

// CM: the 3 x 3 corner of the 3-source layout by a third MFMA instead of the six per-lane
// accumulators (OLPE_NORMAL_CORNER=mfma: the A/B of DESIGN.md §7k; not the default)
template <int NSRC, bool CM = false>
__global__ __launch_bounds__(kWaves * 64) void normal_kernel(
    const double2 *__restrict__ DE, int n, int bkgd_mode, const double *__restrict__ params,
    int W, double *__restrict__ chi2, double *__restrict__ grad, double *__restrict__ jtj) {
  using L = dev::Layout<NSRC>;
  constexpr int P = L::NP, PS = L::PS, S = tile_stride<NSRC>(), HI = P - 16;
  __shared__ double tiles[kWaves][64 * S];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long w = (long long)blockIdx.x * kWaves + wave;
  if (w >= W) return;                          // (wave-uniform; no workgroup barrier below)
  double p[P];
  bool fin = true;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    p[k] = dev::uniform_f64(params[(size_t)w * PS + k]);
    fin = fin && isfinite(p[k]);
  }
  double d[12 * NSRC + 1];
  make_desc<NSRC>(p, bkgd_mode, d);
#pragma unroll
  for (int k = 0; k < 12 * NSRC + 1; ++k) d[k] = dev::uniform_f64(d[k]);
  const Chain<NSRC> ch = make_chain<NSRC>(p);

  double *T = tiles[wave];
  if constexpr (HI > 0) T[lane * S + 19] = 0.0;   // the high operand's zero column
  const int npix = n * n;
  const int rd = (lane >> 4) * S + (lane & 15);
  const int rdh = (lane >> 4) * S + 16 + ((lane & 15) < HI ? (lane & 15) : 3);
  double g[P], hh[HI > 0 ? 6 : 1], chi = 0.0;
#pragma unroll
  for (int k = 0; k < P; ++k) g[k] = 0.0;
#pragma unroll
  for (int k = 0; k < (HI > 0 ? 6 : 1); ++k) hh[k] = 0.0;
  v4d acc = {0.0, 0.0, 0.0, 0.0}, acch = {0.0, 0.0, 0.0, 0.0}, accc = {0.0, 0.0, 0.0, 0.0};
  bool bad = false;
  for (int base = 0; base < npix; base += 64) {
    const int pix = base + lane;
    const bool in = pix < npix;
    const int pc = in ? pix : npix - 1;
    const int i = pc / n, j = pc - i * n;
    const double2 de = DE[pc];
    const bool use = in && de.y != 0.0;
    double J[P];
    const double mod = pixel_jac<NSRC>(d, ch, bkgd_mode, (double)j, (double)i, J);
    bad = bad || (use && !isfinite(mod));
    const double t = (de.x - mod) * de.y;
    const double r = use ? t : 0.0;
    chi = fma(r, r, chi);
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const double jw = J[k] * de.y;
      J[k] = use ? jw : 0.0;
      g[k] = fma(J[k], r, g[k]);
      T[lane * S + k] = J[k];
    }
    if constexpr (HI > 0 && !CM) {
      hh[0] = fma(J[16], J[16], hh[0]);
      hh[1] = fma(J[16], J[17], hh[1]);
      hh[2] = fma(J[16], J[18], hh[2]);
      hh[3] = fma(J[17], J[17], hh[3]);
      hh[4] = fma(J[17], J[18], hh[4]);
      hh[5] = fma(J[18], J[18], hh[5]);
    }
    dev::wave_sync();
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const double a = T[4 * m * S + rd];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
      if constexpr (HI > 0) {
        const double bh = T[4 * m * S + rdh];
        acch = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bh, acch, 0, 0, 0);
        if constexpr (CM) accc = __builtin_amdgcn_mfma_f64_16x16x4f64(bh, bh, accc, 0, 0, 0);
      }
    }
    dev::wave_sync();                          // the tile is rewritten by the next step
  }
  const bool nanout = !fin || __ballot(bad) != 0ull;
  const double nanv = __longlong_as_double(0x7ff8000000000000ll);
  chi = dev::wave_sum(chi);
#pragma unroll
  for (int k = 0; k < P; ++k) g[k] = dev::wave_sum(g[k]);
#pragma unroll
  for (int k = 0; k < (HI > 0 ? 6 : 1); ++k) hh[k] = dev::wave_sum(hh[k]);
  double *oj = jtj + (size_t)w * P * P;
  if (lane == 0) {
    chi2[w] = nanout ? nanv : chi;
#pragma unroll
    for (int k = 0; k < P; ++k) grad[(size_t)w * P + k] = nanout ? nanv : g[k];
    if constexpr (HI > 0 && !CM) {
      constexpr int at[6][2] = {{16, 16}, {16, 17}, {16, 18}, {17, 17}, {17, 18}, {18, 18}};
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const double v = nanout ? nanv : hh[k];
        oj[at[k][0] * P + at[k][1]] = v;
        oj[at[k][1] * P + at[k][0]] = v;
      }
    }
  }
  // C/D of the f64 MFMA: column lane & 15, row (lane >> 4) + 4 reg; the upper triangle goes
  // to both halves
  const int col = lane & 15;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int rowi = (lane >> 4) + 4 * q;
    const double v = nanout ? nanv : acc[q];
    if (rowi <= col) {
      oj[rowi * P + col] = v;
      oj[col * P + rowi] = v;
    }
    if constexpr (HI > 0) {
      const double vh = nanout ? nanv : acch[q];
      if (col < HI) {
        oj[rowi * P + 16 + col] = vh;
        oj[(16 + col) * P + rowi] = vh;
      }
      if constexpr (CM) {
        const double vc = nanout ? nanv : accc[q];
        if (rowi <= col && col < HI) {
          oj[(16 + rowi) * P + 16 + col] = vc;
          oj[(16 + col) * P + 16 + rowi] = vc;
        }
      }
    }
  }
}

// the unweighted derivatives of one vector, a plane per parameter: pixel_jac alone
template <int NSRC>
__global__ __launch_bounds__(kThreads) void jacobian_kernel(const double *__restrict__ vec, int n,
                                                            int bkgd_mode,
                                                            double *__restrict__ planes) {
  using L = dev::Layout<NSRC>;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  const int npix = n * n;
  if (pix >= npix) return;
  double p[L::NP], d[12 * NSRC + 1], J[L::NP];
#pragma unroll
  for (int k = 0; k < L::NP; ++k) p[k] = vec[k];
  make_desc<NSRC>(p, bkgd_mode, d);
  const Chain<NSRC> ch = make_chain<NSRC>(p);
  const int i = pix / n, j = pix - i * n;
  (void)pixel_jac<NSRC>(d, ch, bkgd_mode, (double)j, (double)i, J);
#pragma unroll
  for (int k = 0; k < L::NP; ++k) planes[(size_t)k * npix + pix] = J[k];
}

// the context's two scratch buffers (counted in doubles), grown as olpe_chi2_batch grows them
int reserve(olpe_ctx *c, size_t pin, size_t pout) {
  int rc;
  if (c->scratch_cap < pin) {
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    c->d_scratch = nullptr;
    c->scratch_cap = 0;
    if ((rc = alloc((void **)&c->d_scratch, pin * 8, "the parameter vectors"))) return rc;
    c->scratch_cap = pin;
  }
  if (c->scratch2_cap < pout) {
    if (c->d_scratch2) (void)hipFree(c->d_scratch2);
    c->d_scratch2 = nullptr;
    c->scratch2_cap = 0;
    if ((rc = alloc((void **)&c->d_scratch2, pout * 8, "the normal equations"))) return rc;
    c->scratch2_cap = pout;
  }
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_normal_batch(olpe_ctx *c, const double *params, int W, double *chi2, double *grad,
                      double *jtj) {
  if (!c || !params || !chi2 || !grad || !jtj) return set_err(OLPE_EINVAL, "NULL argument");
  if (W <= 0) return set_err(OLPE_EINVAL, "W must be > 0");
  bool corner_mfma = false;
  if (const char *e = getenv("OLPE_NORMAL_CORNER")) {                       // A/B, tests
    if (strcmp(e, "mfma") && strcmp(e, "valu"))
      return set_err(OLPE_EINVAL, "OLPE_NORMAL_CORNER=%s: mfma or valu", e);
    corner_mfma = !strcmp(e, "mfma");
  }
  HIPCHK(hipSetDevice(c->device));
  const size_t P = (size_t)c->np, nw = (size_t)W;
  const size_t pin = nw * c->ps, pout = nw * (1 + P + P * P);
  int rc;
  HIPCHK(hipStreamSynchronize(olpe_main(c)));     // nothing in flight reads a buffer that grows
  if ((rc = reserve(c, pin, pout))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_scratch, params, pin * 8, hipMemcpyHostToDevice, olpe_main(c)));
  double *d_chi = c->d_scratch2, *d_grad = d_chi + nw, *d_jtj = d_grad + nw * P;
  const dim3 grid((unsigned)((nw + kWaves - 1) / kWaves)), block(kWaves * 64);
  if (c->nsrc == 2)
    hipLaunchKernelGGL((normal_kernel<2>), grid, block, 0, olpe_main(c), c->d_DE, c->n,
                       c->bkgd_mode, c->d_scratch, W, d_chi, d_grad, d_jtj);
  else if (corner_mfma)
    hipLaunchKernelGGL((normal_kernel<3, true>), grid, block, 0, olpe_main(c), c->d_DE, c->n,
                       c->bkgd_mode, c->d_scratch, W, d_chi, d_grad, d_jtj);
  else
    hipLaunchKernelGGL((normal_kernel<3>), grid, block, 0, olpe_main(c), c->d_DE, c->n,
                       c->bkgd_mode, c->d_scratch, W, d_chi, d_grad, d_jtj);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(chi2, d_chi, nw * 8, hipMemcpyDeviceToHost, olpe_main(c)));
  HIPCHK(hipMemcpyAsync(grad, d_grad, nw * P * 8, hipMemcpyDeviceToHost, olpe_main(c)));
  HIPCHK(hipMemcpyAsync(jtj, d_jtj, nw * P * P * 8, hipMemcpyDeviceToHost, olpe_main(c)));
  HIPCHK(hipStreamSynchronize(olpe_main(c)));
  return OLPE_OK;
}

int olpe_test_jacobian(olpe_ctx *c, const double *vec, double *planes) {
  if (!c || !vec || !planes) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  const size_t npix = (size_t)c->n * c->n, pout = (size_t)c->np * npix;
  int rc;
  HIPCHK(hipStreamSynchronize(olpe_main(c)));
  if ((rc = reserve(c, (size_t)c->ps, pout))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_scratch, vec, (size_t)c->ps * 8, hipMemcpyHostToDevice, olpe_main(c)));
  const dim3 grid((unsigned)((npix + kThreads - 1) / kThreads)), block(kThreads);
  if (c->nsrc == 2)
    hipLaunchKernelGGL((jacobian_kernel<2>), grid, block, 0, olpe_main(c), c->d_scratch, c->n,
                       c->bkgd_mode, c->d_scratch2);
  else
    hipLaunchKernelGGL((jacobian_kernel<3>), grid, block, 0, olpe_main(c), c->d_scratch, c->n,
                       c->bkgd_mode, c->d_scratch2);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(planes, c->d_scratch2, pout * 8, hipMemcpyDeviceToHost, olpe_main(c)));
  HIPCHK(hipStreamSynchronize(olpe_main(c)));
  return OLPE_OK;
}

}  // extern "C"
