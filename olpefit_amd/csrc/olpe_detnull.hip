// olpe_detnull.hip -- the false-alarm calibration of the detection map: the null
// distribution of the map's maximum from noise frames drawn on the device.  theta is one
// parameter vector; K_i(c), w_i, Q(c) are olpe_detect.hip's at theta (EXACT operation
// order).  Realisation r of "no further source, Gaussian noise of the frame's own err":
//   eps_r  = np.random.RandomState((seed + r) mod 2^32).standard_normal(n * n) in raster
//            order (MT19937, init_genrand, the legacy polar gauss); every pixel takes a draw;
//   y_r,i  = eps_r,i (1 / err_i), 0 at masked pixels (the 1 / err the context staged);
//   snr_r(c) = scale(c) ((sum_i K_i(c) y_r,i) / sqrt(Q(c))), NaN where Q(c) = 0.
// Each map is reduced on the device to its maximum (all candidates, and those farther than
// exclude_px from every fitted source), its number of strict local maxima at or above a
// threshold (detect.candidates' rule) and the maximum of every ring of the contrast curve.
//
// An olpe_detect_null copies from an olpe_detect, evaluated once at theta, the slot-0 PSF
// tables, the staged cutout and the Q plane; it is independent of the olpe_detect and of the
// context afterwards.  A batch of at most B realisations goes through
//   1. noise    a wave per realisation: the MT19937 key in LDS, seeded serially
//               (mt_seed_serial), twisted lane-parallel; the 156 polar attempts of a key (pair
//               k = words 4k .. 4k + 3) are evaluated lane-parallel, accepted per pair, and an
//               accepted pair writes f x2 then f x1 at the position the prefix count of the
//               accepts gives.  x1 x1 + x2 x2 is not contracted (-ffp-contract=off);
//   2. weight   y [n^2][Bp], realisation-fastest, Bp = B rounded up to 32, zero beyond the
//               batch's count;
//   3. corr     the hot path, G n^2 FMAs per realisation from the ONE table set of theta.  A
//               workgroup takes 64 candidate columns, kRR candidate rows, a phase and 32
//               realisations, a wave 8 of them: a lane holds kRR x 8 sums.  The workgroup
//               walks the pixel rows through LDS, kPD at a time with the kPD + kRR - 1 table
//               rows they meet; per pixel, kRR LDS reads of the table (Toeplitz: column
//               ix - cx) and one scalar load of 8 realisations' y feed 8 kRR FMAs.  A
//               candidate's sum runs over the pixels row by row, column by column: the order
//               is the frame's, not the batch's.  The epilogue applies scale / sqrt(Q);
//   4. stats    a workgroup per realisation: maxima with the first index on ties, peaks,
//               ring maxima (integer LDS maxima of order-preserving keys).
// No floating-point atomics.  DESIGN.md §7m has the layout and the measurements.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/olpe.h"
#include "olpe_fold.h"
#include "olpe_internal.h"

// the sampler's MT19937 pieces, by #include only (see olpe_resid.hip)
namespace olpe_detnull_dev {
#include "olpe_device.h"
}
namespace dev = olpe_detnull_dev::olpe;

using namespace olpe;

struct olpe_detect_null : FoldBase {
  int n = 0, os = 1, gs = 0, ps = 17;
  int B = 0, Bp = 0;            // realisations per batch, and rounded up to kGroup
  int nring = 0;
  int mode = 0;                 // kNone, kGenerated, kFrames
  size_t npix = 0, G = 0, tabs = 0;
  double threshold = 5.0;
  unsigned long long seed = 0;
  long long done = 0;
  double *d_tab = nullptr;      // [os^2][2n - 1][2n - 1] the tables of theta
  double2 *d_DE = nullptr;      // [npix] the staged cutout
  double *d_Q = nullptr;        // [G]
  double *d_scale = nullptr;    // [G]
  int *d_ring = nullptr;        // [G] ring of each candidate
  unsigned char *d_outside = nullptr;   // [G] 1: farther than exclude_px from every source
  double *d_eps = nullptr;      // [B][npix]
  double *d_y = nullptr;        // [npix][Bp]
  double *d_map = nullptr;      // [B][G]
  double *d_resd = nullptr;     // [B][2 + nring] max_all, max_out, ring_max
  long long *d_resi = nullptr;  // [B][4] argmax_all, argmax_out, peaks_all, peaks_out
  std::vector<double> max_all, max_out, ring_max;
  std::vector<long long> arg_all, arg_out, peaks_all, peaks_out;
};

namespace {

enum { kNone = 0, kGenerated = 1, kFrames = 2 };
constexpr int kThreads = 256;
constexpr int kRR = 4;          // candidate rows of a workgroup of the correlation
constexpr int kRB = 8;          // realisations of a wave
constexpr int kNW = 4;          // waves of a workgroup: realisation blocks
constexpr int kGroup = kRB * kNW;
constexpr int kPD = 8;          // pixel rows staged at a time
constexpr int kSegRows = kPD + kRR - 1;
constexpr int kSegW = 192;      // n + 63 table columns of a tile, n <= 128
constexpr int kMaxSide = 128;   // olpe_detect's
static_assert(kMaxSide + 63 <= kSegW, "a tile's table columns fit a row of the LDS segment");
constexpr int kMaxRings = 2048;
constexpr int kMaxBatch = 4096;
constexpr size_t kWorkBudget = 512u << 20;   // bytes of per-realisation buffers a batch aims at

// 1. noise: workgroup = wave = realisation r0 + blockIdx.x
__global__ __launch_bounds__(64) void detnull_noise_kernel(unsigned long long seed, long long r0,
                                                           int npix, double *__restrict__ eps) {
  __shared__ uint32_t key[dev::MT_N];
  const int lane = threadIdx.x;
  double *out = eps + (size_t)blockIdx.x * npix;
  if (lane == 0) dev::mt_seed_serial(key, (uint32_t)(seed + (unsigned long long)(r0 + blockIdx.x)));
  __syncthreads();
  int count = 0;
  while (count < npix) {
    // numpy's mt19937_gen, 64 words at a time: word i takes the old words i, i + 1 and
    // i + 397 (i < 227) or the new word i - 227, written by an earlier pass; the last word
    // takes the new words 0 and 396
    for (int p = 0; p < 10; ++p) {
      const int i = 64 * p + lane;
      uint32_t nv = 0;
      if (i < dev::MT_N) {
        const uint32_t a = key[i], b = key[i + 1 < dev::MT_N ? i + 1 : 0];
        const uint32_t s = i < dev::MT_N - dev::MT_M ? key[i + dev::MT_M]
                                                     : key[i - (dev::MT_N - dev::MT_M)];
        const uint32_t y = (a & dev::MT_UP) | (b & dev::MT_LO);
        nv = s ^ (y >> 1) ^ ((y & 1u) ? dev::MT_A : 0u);
      }
      __syncthreads();
      if (i < dev::MT_N) key[i] = nv;
      __syncthreads();
    }
    // the key's 156 polar attempts
    for (int j = 0; j < 3 && count < npix; ++j) {
      const int k = 64 * j + lane;
      bool ok = false;
      double g2 = 0.0, g1 = 0.0;
      if (k < dev::MT_N / 4) {
        const uint32_t w0 = dev::mt_temper(key[4 * k]), w1 = dev::mt_temper(key[4 * k + 1]);
        const uint32_t w2 = dev::mt_temper(key[4 * k + 2]), w3 = dev::mt_temper(key[4 * k + 3]);
        const double u1 = ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0;
        const double u2 = ((double)(w2 >> 5) * 67108864.0 + (double)(w3 >> 6)) / 9007199254740992.0;
        const double x1 = 2.0 * u1 - 1.0;
        const double x2 = 2.0 * u2 - 1.0;
        const double r2 = x1 * x1 + x2 * x2;
        ok = r2 < 1.0 && r2 != 0.0;
        if (ok) {
          const double f = sqrt(-2.0 * log(r2) / r2);
          g2 = f * x2;
          g1 = f * x1;
        }
      }
      const unsigned long long bal = __ballot(ok);
      const int pos = count + 2 * __popcll(bal & ((1ull << lane) - 1ull));
      if (ok) {
        if (pos < npix) out[pos] = g2;
        if (pos + 1 < npix) out[pos + 1] = g1;     // else the cached deviate, discarded
      }
      count += 2 * __popcll(bal);
    }
  }
}

// 2. weight: thread = (pixel, realisation of the padded batch)
__global__ __launch_bounds__(kThreads) void detnull_weight_kernel(
    const double *__restrict__ eps, const double2 *__restrict__ DE, size_t npix, int count, int Bp,
    double *__restrict__ y) {
  const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= npix * (size_t)Bp) return;
  const size_t i = t / Bp;
  const int r = (int)(t - i * Bp);
  const double ie = DE[i].y;
  y[t] = r < count && ie != 0.0 ? eps[(size_t)r * npix + i] * ie : 0.0;
}

// 3. corr: workgroup (x, y, z) = tile x (64 candidate columns, kRR candidate rows), phase y,
// realisations 32 z ..; wave w of it the realisations 32 z + 8 w ...  Pixel row iy meets
// candidate row cy at table row d = iy - cy.  seg[j][k]: table row iy0 - cy0 - (kRR - 1) + j,
// column k - 63 - cx0 (0 outside the table), so lane l reads seg[a - rr + kRR - 1][63 - l + ix]
// for pixel (iy0 + a, ix) and candidate row cy0 + rr.
__global__ __launch_bounds__(64 * kNW) __attribute__((amdgpu_waves_per_eu(4, 8)))
void detnull_corr_kernel(const double *__restrict__ tab, const double *__restrict__ y,
                         const double *__restrict__ Q, const double *__restrict__ scale, int n,
                         int os, int gs, int count, int Bp, double *__restrict__ map) {
  __shared__ double seg[kSegRows][kSegW];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tx = (n + 63) >> 6;
  const int trow = blockIdx.x / tx, tcol = blockIdx.x - trow * tx;
  const int ph = blockIdx.y, py = ph / os, px = ph - py * os;
  const int T = 2 * n - 1, W = n + 63;
  const double *P = tab + (size_t)ph * T * T;
  const int cx0 = tcol * 64, cy0 = trow * kRR;
  const int r0 = __builtin_amdgcn_readfirstlane((int)blockIdx.z * kGroup + wave * kRB);
  double acc[kRR][kRB];
#pragma unroll
  for (int rr = 0; rr < kRR; ++rr)
#pragma unroll
    for (int b = 0; b < kRB; ++b) acc[rr][b] = 0.0;
  for (int iy0 = 0; iy0 < n; iy0 += kPD) {
    const int dbase = iy0 - cy0 - (kRR - 1);
    __syncthreads();
    for (int k = threadIdx.x; k < kSegRows * W; k += 64 * kNW) {
      const int j = k / W, col = k - j * W;
      const int tr = dbase + j + n - 1, tc = col - 63 - cx0 + n - 1;
      seg[j][col] = tr >= 0 && tr < T && tc >= 0 && tc < T ? P[(size_t)tr * T + tc] : 0.0;
    }
    __syncthreads();
    const int na = min(kPD, n - iy0);
    for (int a = 0; a < na; ++a) {
      const double *yr = y + ((size_t)(iy0 + a) * n) * Bp + r0;
      const double *sp = &seg[a + kRR - 1][63 - lane];
#pragma unroll 2
      for (int ix = 0; ix < n; ++ix) {
        double p[kRR];
#pragma unroll
        for (int rr = 0; rr < kRR; ++rr) p[rr] = sp[ix - rr * kSegW];
        const double *ys = yr + (size_t)ix * Bp;
#pragma unroll
        for (int b = 0; b < kRB; ++b) {
          const double yv = ys[b];
#pragma unroll
          for (int rr = 0; rr < kRR; ++rr) acc[rr][b] = fma(p[rr], yv, acc[rr][b]);
        }
      }
    }
  }
  const size_t G = (size_t)gs * gs;
  const int cx = cx0 + lane, jx = os * cx + px;
#pragma unroll
  for (int rr = 0; rr < kRR; ++rr) {
    const int cy = cy0 + rr, jy = os * cy + py;
    if (cx < n && cy < n && jx < gs && jy < gs) {
      const size_t g = (size_t)jy * gs + jx;
      const double q = Q[g], sc = scale[g];
      const double rq = q > 0.0 ? sqrt(q) : 0.0;
#pragma unroll
      for (int b = 0; b < kRB; ++b)
        if (r0 + b < count) map[(size_t)(r0 + b) * G + g] = q > 0.0 ? sc * (acc[rr][b] / rq) : nan("");
    }
  }
}

// an unsigned key in the order of the doubles that are no NaN; 0 is below every one
__device__ __forceinline__ unsigned long long order_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double key_value(unsigned long long k) {
  if (k == 0) return nan("");
  return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

// the better of two (value, index) maxima: the larger value, the lower index on a tie; an
// index of -1 is no candidate
__device__ __forceinline__ void take_max(double &v, long long &at, double v2, long long at2) {
  if (at2 >= 0 && (at < 0 || v2 > v || (v2 == v && at2 < at))) {
    v = v2;
    at = at2;
  }
}

// 4. stats: workgroup = realisation
__global__ __launch_bounds__(kThreads) void detnull_stats_kernel(
    const double *__restrict__ map, const int *__restrict__ ring,
    const unsigned char *__restrict__ outside, int gs, int nring, double threshold,
    double *__restrict__ resd, long long *__restrict__ resi) {
  __shared__ unsigned long long s_ring[kMaxRings];
  __shared__ double s_v[2][kThreads];
  __shared__ long long s_at[2][kThreads];
  __shared__ int s_peaks[2];
  const int t = threadIdx.x;
  const size_t G = (size_t)gs * gs;
  const double *m = map + (size_t)blockIdx.x * G;
  for (int k = t; k < nring; k += kThreads) s_ring[k] = 0;
  if (t < 2) s_peaks[t] = 0;
  __syncthreads();
  double v_all = 0.0, v_out = 0.0;
  long long at_all = -1, at_out = -1;
  int pk_all = 0, pk_out = 0;
  for (size_t g = t; g < G; g += kThreads) {
    const double v = m[g];
    if (v != v) continue;
    const bool out = outside[g] != 0;
    take_max(v_all, at_all, v, (long long)g);
    if (out) take_max(v_out, at_out, v, (long long)g);
    atomicMax(&s_ring[ring[g]], order_key(v));
    if (!(v >= threshold)) continue;
    const int jy = (int)(g / gs), jx = (int)(g - (size_t)jy * gs);
    bool peak = true;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = jy + dy, xx = jx + dx;
        if ((dy || dx) && yy >= 0 && yy < gs && xx >= 0 && xx < gs) {
          const double nb = m[(size_t)yy * gs + xx];
          if (nb == nb && !(v > nb)) peak = false;
        }
      }
    pk_all += peak;
    pk_out += peak && out;
  }
  s_v[0][t] = v_all;
  s_at[0][t] = at_all;
  s_v[1][t] = v_out;
  s_at[1][t] = at_out;
  if (pk_all) atomicAdd(&s_peaks[0], pk_all);
  if (pk_out) atomicAdd(&s_peaks[1], pk_out);
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if (t < h)
      for (int k = 0; k < 2; ++k) take_max(s_v[k][t], s_at[k][t], s_v[k][t + h], s_at[k][t + h]);
    __syncthreads();
  }
  double *od = resd + (size_t)blockIdx.x * (2 + nring);
  long long *oi = resi + (size_t)blockIdx.x * 4;
  if (t < 2) {
    od[t] = s_at[t][0] >= 0 ? s_v[t][0] : nan("");
    oi[t] = s_at[t][0];
    oi[2 + t] = s_peaks[t];
  }
  for (int k = t; k < nring; k += kThreads) od[2 + k] = key_value(s_ring[k]);
}

unsigned blocks_of(size_t len) { return (unsigned)((len + kThreads - 1) / kThreads); }

bool all_finite(const double *v, size_t len) {
  for (size_t i = 0; i < len; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

void launch_noise(olpe_detect_null *h, long long r0, int count) {
  hipLaunchKernelGGL(detnull_noise_kernel, dim3((unsigned)count), dim3(64), 0, h->stream, h->seed,
                     r0, (int)h->npix, h->d_eps);
}

// steps 2 - 3 on the first `count` frames of d_eps
void launch_maps(olpe_detect_null *h, int count) {
  const int groups = (count + kGroup - 1) / kGroup;
  const int tiles = ((h->n + 63) / 64) * ((h->n + kRR - 1) / kRR);
  hipLaunchKernelGGL(detnull_weight_kernel, dim3(blocks_of(h->npix * (size_t)h->Bp)),
                     dim3(kThreads), 0, h->stream, h->d_eps, h->d_DE, h->npix, count, h->Bp, h->d_y);
  hipLaunchKernelGGL(detnull_corr_kernel,
                     dim3((unsigned)tiles, (unsigned)(h->os * h->os), (unsigned)groups),
                     dim3(64 * kNW), 0, h->stream, h->d_tab, h->d_y, h->d_Q, h->d_scale, h->n, h->os,
                     h->gs, count, h->Bp, h->d_map);
}

// step 4 on the batch's maps, and its results behind the object's
int reduce_batch(olpe_detect_null *h, int count) {
  hipLaunchKernelGGL(detnull_stats_kernel, dim3((unsigned)count), dim3(kThreads), 0, h->stream,
                     h->d_map, h->d_ring, h->d_outside, h->gs, h->nring, h->threshold, h->d_resd,
                     h->d_resi);
  HIPCHK(hipGetLastError());
  const size_t wd = 2 + (size_t)h->nring;
  std::vector<double> rd((size_t)count * wd);
  std::vector<long long> ri((size_t)count * 4);
  HIPCHK(hipMemcpyAsync(rd.data(), h->d_resd, rd.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ri.data(), h->d_resi, ri.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int r = 0; r < count; ++r) {
    h->max_all.push_back(rd[r * wd]);
    h->max_out.push_back(rd[r * wd + 1]);
    h->ring_max.insert(h->ring_max.end(), rd.begin() + r * wd + 2, rd.begin() + (r + 1) * wd);
    h->arg_all.push_back(ri[(size_t)r * 4]);
    h->arg_out.push_back(ri[(size_t)r * 4 + 1]);
    h->peaks_all.push_back(ri[(size_t)r * 4 + 2]);
    h->peaks_out.push_back(ri[(size_t)r * 4 + 3]);
  }
  h->done += count;
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_detect_null_create(olpe_detect *d, const double *vec, const double *scale,
                            const double *known, int nknown, double exclude_px,
                            const double *centre, double bin_px, double threshold,
                            unsigned long long seed, int batch, olpe_detect_null **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (!d || !vec || !centre || (nknown > 0 && !known)) return set_err(OLPE_EINVAL, "NULL argument");
  olpe_detect_view v;
  int rc;
  if ((rc = olpe_detect_view_at(d, nullptr, &v))) return rc;
  const size_t G = (size_t)v.gs * v.gs, npix = (size_t)v.n * v.n;
  if (!all_finite(vec, (size_t)v.ps - 1))
    return set_err(OLPE_EINVAL, "the vector has a non-finite parameter");
  if (scale)
    for (size_t g = 0; g < G; ++g)
      if (!std::isfinite(scale[g]) || scale[g] <= 0.0)
        return set_err(OLPE_EINVAL, "scale %g at candidate %zu: finite and > 0", scale[g], g);
  if (nknown < 0 || !all_finite(known, 2 * (size_t)std::max(nknown, 0)) || !all_finite(centre, 2))
    return set_err(OLPE_EINVAL, "%d known sources; their and the centre's coordinates are finite",
                   nknown);
  if (!std::isfinite(exclude_px) || exclude_px < 0.0 || !std::isfinite(bin_px) || bin_px <= 0.0 ||
      threshold != threshold)
    return set_err(OLPE_EINVAL, "exclude_px %g (>= 0), bin_px %g (> 0), threshold %g", exclude_px,
                   bin_px, threshold);
  if (batch < 0 || batch > kMaxBatch)
    return set_err(OLPE_EINVAL, "batch %d: 0 (from the byte budget) .. %d", batch, kMaxBatch);
  // the rings of detect.contrast_curve and the flag of detect.candidates, in their arithmetic
  std::vector<int> ring(G);
  std::vector<unsigned char> outside(G);
  int nring = 0;
  for (int jy = 0; jy < v.gs; ++jy)
    for (int jx = 0; jx < v.gs; ++jx) {
      const double x = (double)jx / (double)v.os, y = (double)jy / (double)v.os;
      const double k = floor(hypot(x - centre[0], y - centre[1]) / bin_px);
      if (!(k < (double)kMaxRings))
        return set_err(OLPE_EINVAL, "bin_px %g: more than %d rings", bin_px, kMaxRings);
      const size_t g = (size_t)jy * v.gs + jx;
      ring[g] = (int)k;
      nring = std::max(nring, (int)k + 1);
      bool near = false;
      for (int s = 0; s < nknown; ++s)
        near = near || hypot(x - known[2 * s], y - known[2 * s + 1]) <= exclude_px;
      outside[g] = !near;
    }
  // theta's tables, Q and the cutout, from here on GPU calls
  if ((rc = olpe_detect_view_at(d, vec, &v))) return rc;
  olpe_detect_null *h = new olpe_detect_null;
  h->n = v.n;
  h->os = v.os;
  h->gs = v.gs;
  h->ps = v.ps;
  h->npix = npix;
  h->G = G;
  h->tabs = v.tabs;
  h->nring = nring;
  h->threshold = threshold;
  h->seed = seed;
  const size_t per = 2 * npix * 8 + G * 8;
  h->B = batch ? batch
               : (int)std::min<size_t>(kMaxBatch, std::max<size_t>(kGroup, kWorkBudget / per / kGroup * kGroup));
  h->Bp = (h->B + kGroup - 1) / kGroup * kGroup;
  std::vector<double> ones;
  if (!scale) ones.assign(G, 1.0);
  rc = fold_open(h, v.device);
  if (!rc) rc = alloc((void **)&h->d_tab, h->tabs * 8, "the PSF tables");
  if (!rc) rc = alloc((void **)&h->d_DE, npix * sizeof(double2), "the cutout");
  if (!rc) rc = alloc((void **)&h->d_Q, G * 8, "the Q plane");
  if (!rc) rc = alloc((void **)&h->d_scale, G * 8, "the scale plane");
  if (!rc) rc = alloc((void **)&h->d_ring, G * sizeof(int), "the rings");
  if (!rc) rc = alloc((void **)&h->d_outside, G, "the exclusion flags");
  if (!rc) rc = alloc((void **)&h->d_eps, (size_t)h->B * npix * 8, "the noise frames");
  if (!rc) rc = alloc((void **)&h->d_y, npix * (size_t)h->Bp * 8, "the weighted frames");
  if (!rc) rc = alloc((void **)&h->d_map, (size_t)h->B * G * 8, "the maps");
  if (!rc) rc = alloc((void **)&h->d_resd, (size_t)h->B * (2 + (size_t)nring) * 8, "the results");
  if (!rc) rc = alloc((void **)&h->d_resi, (size_t)h->B * 4 * 8, "the results");
  if (!rc && (hipMemcpy(h->d_tab, v.tab, h->tabs * 8, hipMemcpyDeviceToDevice) != hipSuccess ||
              hipMemcpy(h->d_DE, v.DE, npix * sizeof(double2), hipMemcpyDeviceToDevice) != hipSuccess ||
              hipMemcpy(h->d_Q, v.Q, G * 8, hipMemcpyDeviceToDevice) != hipSuccess ||
              hipMemcpy(h->d_scale, scale ? scale : ones.data(), G * 8, hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(h->d_ring, ring.data(), G * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(h->d_outside, outside.data(), G, hipMemcpyHostToDevice) != hipSuccess ||
              hipDeviceSynchronize() != hipSuccess))
    rc = set_err(OLPE_EHIP, "copying the tables failed");
  if (rc) {
    olpe_detect_null_destroy(h);
    return rc;
  }
  *out = h;
  return OLPE_OK;
}

void olpe_detect_null_destroy(olpe_detect_null *h) {
  if (!h) return;
  fold_close(h, {h->d_tab, h->d_DE, h->d_Q, h->d_scale, h->d_ring, h->d_outside, h->d_eps, h->d_y,
                 h->d_map, h->d_resd, h->d_resi});
  delete h;
}

int olpe_detect_null_run(olpe_detect_null *h, long long count) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  if (count < 0) return set_err(OLPE_EINVAL, "count %lld", count);
  if (h->mode == kFrames)
    return set_err(OLPE_ESTATE, "this object holds realisations of explicit frames: reset it "
                   "before generating");
  if (count == 0) return OLPE_OK;
  HIPCHK(hipSetDevice(h->device));
  h->mode = kGenerated;
  for (long long k = 0; k < count; k += h->B) {
    const int c = (int)std::min<long long>(h->B, count - k);
    launch_noise(h, h->done, c);
    launch_maps(h, c);
    int rc;
    if ((rc = reduce_batch(h, c))) return rc;
  }
  return OLPE_OK;
}

int olpe_detect_null_run_frames(olpe_detect_null *h, const double *eps, long long count) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  if (count < 0 || (count > 0 && !eps))
    return set_err(OLPE_EINVAL, "%lld frames at %p", count, (const void *)eps);
  if (h->mode == kGenerated)
    return set_err(OLPE_ESTATE, "this object holds generated realisations: reset it before "
                   "passing explicit frames");
  if (count == 0) return OLPE_OK;
  HIPCHK(hipSetDevice(h->device));
  h->mode = kFrames;
  for (long long k = 0; k < count; k += h->B) {
    const int c = (int)std::min<long long>(h->B, count - k);
    HIPCHK(hipMemcpyAsync(h->d_eps, eps + (size_t)k * h->npix, (size_t)c * h->npix * 8,
                          hipMemcpyHostToDevice, h->stream));
    launch_maps(h, c);
    int rc;
    if ((rc = reduce_batch(h, c))) return rc;
  }
  return OLPE_OK;
}

int olpe_detect_null_get(olpe_detect_null *h, long long *done, int *nring, double *max_all,
                         long long *argmax_all, double *max_out, long long *argmax_out,
                         long long *peaks_all, long long *peaks_out, double *ring_max) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  const size_t R = (size_t)h->done;
  if (done) *done = h->done;
  if (nring) *nring = h->nring;
  if (R) {
    if (max_all) memcpy(max_all, h->max_all.data(), R * 8);
    if (argmax_all) memcpy(argmax_all, h->arg_all.data(), R * 8);
    if (max_out) memcpy(max_out, h->max_out.data(), R * 8);
    if (argmax_out) memcpy(argmax_out, h->arg_out.data(), R * 8);
    if (peaks_all) memcpy(peaks_all, h->peaks_all.data(), R * 8);
    if (peaks_out) memcpy(peaks_out, h->peaks_out.data(), R * 8);
    if (ring_max) memcpy(ring_max, h->ring_max.data(), R * h->nring * 8);
  }
  return OLPE_OK;
}

int olpe_detect_null_maps(olpe_detect_null *h, long long r0, long long count, double *out) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  if (r0 < 0 || count < 0 || (count > 0 && !out))
    return set_err(OLPE_EINVAL, "realisations %lld .. + %lld at %p", r0, count, (void *)out);
  if (h->mode == kFrames)
    return set_err(OLPE_ESTATE, "this object holds realisations of explicit frames");
  HIPCHK(hipSetDevice(h->device));
  for (long long k = 0; k < count; k += h->B) {
    const int c = (int)std::min<long long>(h->B, count - k);
    launch_noise(h, r0 + k, c);
    launch_maps(h, c);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out + (size_t)k * h->G, h->d_map, (size_t)c * h->G * 8,
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return OLPE_OK;
}

int olpe_detect_null_noise(olpe_detect_null *h, long long r0, long long count, double *out) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  if (r0 < 0 || count < 0 || (count > 0 && !out))
    return set_err(OLPE_EINVAL, "realisations %lld .. + %lld at %p", r0, count, (void *)out);
  if (h->mode == kFrames)
    return set_err(OLPE_ESTATE, "this object holds realisations of explicit frames");
  HIPCHK(hipSetDevice(h->device));
  for (long long k = 0; k < count; k += h->B) {
    const int c = (int)std::min<long long>(h->B, count - k);
    launch_noise(h, r0 + k, c);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out + (size_t)k * h->npix, h->d_eps, (size_t)c * h->npix * 8,
                          hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return OLPE_OK;
}

int olpe_detect_null_reset(olpe_detect_null *h) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->done = 0;
  h->mode = kNone;
  for (auto *v : {&h->max_all, &h->max_out, &h->ring_max}) v->clear();
  for (auto *v : {&h->arg_all, &h->arg_out, &h->peaks_all, &h->peaks_out}) v->clear();
  return OLPE_OK;
}

}  // extern "C"
