// olpe_lik.hip -- the posterior's pointwise deviance, folded on the device: how well the
// model predicts every pixel over the whole ensemble (WAIC, DIC), which the reference, whose
// chi^2 column (apf_step2.py:134-148; 3body/apf_step2_3body.py:134-148) is only plotted,
// cannot say.  Every sample's model is build_analytical_model (apf_step2.py:106-124; 3body
// :106-125) in the EXACT operation order, whatever the context's eval mode.
//
// For an unmasked pixel i and a usable row s:  t = (D_i - M_is) * w_i with w the staged
// 1 / err, x = t * t (a rounded product).  log p(D_i | theta_s) = -x / 2 + k_i; k_i = log w_i
// - log(2 pi) / 2 is left out of the planes and reported once, summed (log_norm).  An
// olpe_lik copies a context's staged cutout and keeps, per pixel, about the plane c = x of
// a pivot vector:  A1 = sum (x - c),  A2 = sum (x - c)^2,  and the running log-sum-exp
// pair  m = min x,  L = sum exp(-(x - m) / 2)  (empty: +inf, 0).  Two pairs merge by
// m' = min, L' = L_a exp(-(m_a - m') / 2) + L_b exp(-(m_b - m') / 2), the factor of the
// side that holds the minimum being exactly 1 and an empty side skipped (lse_merge): the
// rule of the block partials, in block order, and of olpe_lik_add.
//
// A piece of at most piece_blocks * kB samples goes through olpe_resid.hip's six launches
// (scan, book, desc shared through olpe_samples.h): the pivot launch writes c, the fold
// kernel holds four accumulators per pixel and writes part[block][4][npix], the reduce
// kernel adds A1 and A2 and merges (m, L) in block order.  No floating-point atomics; a
// pixel's state takes the same operations in the same order for any grid, CU count or
// tile height.
//
// A sample whose t is not finite at a pixel (a model that overflows) is not dropped at
// that pixel the way np.ma would drop it: the pixel's sums become non-finite, finalize
// writes NaN into its planes, leaves it out of every total and counts it (poisoned).
// Masked pixels are staged {0, 0}: they accumulate zeros without a branch and finalize
// writes NaN there.  DESIGN.md §7j has the layout and the measurements.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/olpe.h"
#include "olpe_fold.h"
#include "olpe_internal.h"

// The sampler's device functions, by #include only (see olpe_resid.hip).
namespace olpe_lik_dev {
#include "olpe_device.h"
}
namespace dev = olpe_lik_dev::olpe;

using namespace olpe;

// scan, book, desc and the per-pixel model, shared with olpe_resid.hip
#include "olpe_samples.h"

struct olpe_lik : FoldBase {
  int n = 0, nsrc = 2, np = 16, bkgd_mode = 0, ps = 17;
  int rows = 8;                 // tile height of the fold kernel (4 or 8)
  int piece_blocks = 0;         // blocks of kB samples per piece
  size_t npix = 0;
  bool explicit_pivot = false;  // the pivot came with olpe_lik_create
  double2 *d_DE = nullptr;      // [npix] the context's staged cutout
  double *d_sum = nullptr;      // [4][npix] A1, A2, m, L
  double *d_cimg = nullptr;     // [npix] c
  double *d_pivot = nullptr;    // [ps]
  double *d_best = nullptr;     // [ps]
  double *d_vec = nullptr;      // [ps] the vector of point / finalize
  unsigned long long *d_words = nullptr;  // [kWords]
  void *d_info = nullptr;       // [piece_blocks] BlkInfo
  int *d_boff = nullptr;        // [piece_blocks] compact offset of each block
  double *d_desc = nullptr;     // [piece_blocks * kB][6 G + 1]
  double *d_part = nullptr;     // [piece_blocks][4][npix]
  double *d_planes = nullptr;   // [OLPE_LIK_PLANES][npix]
  void *d_fin = nullptr;        // [ceil(npix / 256)] FinPart
  double *d_stage = nullptr;    // upload staging of fold_rows (allocated on first use)
};

namespace {

struct FinPart {
  double lppd, pwaic, elpd, mean, best, at, lognorm;
  int cnt, poisoned, high;
};

// the deviance x of the model d at pixel (column j, row i) of the staged cutout
template <int NSRC>
__device__ __forceinline__ double pixel_dev(const double *d, int j, int i, double2 de) {
  const double t = (de.x - pixel_model<NSRC>(d, (double)j, (double)i)) * de.y;
  return t * t;
}

// (m, L) <- (m, L) merged with (mb, Lb); one exp: the minimum's side keeps the factor 1
__device__ __forceinline__ void lse_merge(double &m, double &L, double mb, double Lb) {
  if (mb == INFINITY && Lb == 0.0) return;        // nothing to add
  if (m == INFINITY && L == 0.0) {
    m = mb;
    L = Lb;
    return;
  }
  const double f = dev::exp_neg(fabs(m - mb) * 0.5);
  if (mb < m) {
    L = L * f + Lb;
    m = mb;
  } else {
    L = L + Lb * f;
  }
}

// 3. pivot: c = x of the pivot vector, when the book kernel took one (or `force`)
template <int NSRC>
__global__ __launch_bounds__(kThreads) void lik_pivot_kernel(
    const unsigned long long *__restrict__ words, int force, const double *__restrict__ pivot,
    const double2 *__restrict__ DE, int n, int bkgd_mode, double *__restrict__ img) {
  if (!force && !words[kWPivotNew]) return;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= n * n) return;
  double d[12 * NSRC + 1];
  make_desc<NSRC>(pivot, bkgd_mode, d);
  const int i = pix / n, j = pix - i * n;
  img[pix] = pixel_dev<NSRC>(d, j, i, DE[pix]);
}

// x of one vector, NaN at masked pixels
template <int NSRC>
__global__ __launch_bounds__(kThreads) void lik_point_kernel(
    const double *__restrict__ vec, const double2 *__restrict__ DE, int n, int bkgd_mode,
    double *__restrict__ img) {
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= n * n) return;
  double d[12 * NSRC + 1];
  make_desc<NSRC>(vec, bkgd_mode, d);
  const int i = pix / n, j = pix - i * n;
  const double2 de = DE[pix];
  img[pix] = de.y == 0.0 ? nan("") : pixel_dev<NSRC>(d, j, i, de);
}

// 5. fold: workgroup (x, y) = tile y, blocks 4 x .. 4 x + 3 of the piece, a wave each.
// Lanes beyond column n - 1 compute the last column, a tile's rows beyond n - 1 are
// computed like the others against {0, 0} (no branch in the row loop); neither is stored.
// part[block][4][npix].
template <int NSRC, int R>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void lik_fold_kernel(const double *__restrict__ desc,
                     const unsigned long long *__restrict__ words,
                     const double2 *__restrict__ DE, const double *__restrict__ cimg, int n,
                     double *__restrict__ part) {
  constexpr int G = 2 * NSRC, KS = 6 * G + 1;
  static_assert(KS <= 64, "a lane per double of the descriptor");
  __shared__ double sD[R * 64], sW[R * 64], sC[R * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = (n + 63) >> 6;
  const int trow = blockIdx.y / tx, tcol = blockIdx.y - trow * tx;
  const int j = tcol * 64 + lane, r0 = trow * R;
  const bool act = j < n;
  const int jj = act ? j : n - 1;
  for (int k = wave; k < R; k += kThreads / 64) {
    const bool in = r0 + k < n;
    const double2 de = in ? DE[(size_t)(r0 + k) * n + jj] : make_double2(0.0, 0.0);
    sD[k * 64 + lane] = de.x;
    sW[k * 64 + lane] = de.y;
    sC[k * 64 + lane] = in ? cimg[(size_t)(r0 + k) * n + jj] : 0.0;
  }
  __syncthreads();
  const long long cnt = (long long)words[kWPiece];
  const long long blk = (long long)blockIdx.x * (kThreads / 64) + wave;
  if (blk * kB >= cnt) return;
  const int ns = (int)(cnt - blk * kB < kB ? cnt - blk * kB : kB);
  const double *d = desc + (size_t)blk * kB * KS + (lane < KS ? lane : 0);
  const double xj = (double)jj;
  double a1[R], a2[R], mn[R], ls[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    a1[k] = a2[k] = ls[k] = 0.0;
    mn[k] = INFINITY;
  }
  double cur = d[0];
  for (int s = 0; s < ns; ++s) {
    const double nxt = d[(size_t)(s + 1 < ns ? s + 1 : s) * KS];   // the next sample's, ahead
    double amp[G], y0[G], kc[G], t1[G], t2[G];
    dev::static_for<G>([&](auto gi) {
      constexpr int g = decltype(gi)::value;
      amp[g] = bcast_lane<6 * g>(cur);
      y0[g] = bcast_lane<6 * g + 2>(cur);
      kc[g] = bcast_lane<6 * g + 5>(cur);
      const double xd = xj - bcast_lane<6 * g + 1>(cur);
      t1[g] = bcast_lane<6 * g + 3>(cur) * (xd * xd);
      t2[g] = bcast_lane<6 * g + 4>(cur) * xd;
    });
    const double bg = bcast_lane<6 * G>(cur);
    // (the row numbers are converted per sample: hoisted, they would take 2R registers)
    int rr = r0;
    asm volatile("" : "+s"(rr));
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const double yi = (double)(rr + k);
      double v[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const double yd = yi - y0[g];
        const double qq = (t1[g] + t2[g] * yd) + kc[g] * (yd * yd);
        v[g] = amp[g] * dev::exp_neg(qq);
      }
      double mod = v[0] + v[1];
#pragma unroll
      for (int q = 1; q < NSRC; ++q) mod = mod + (v[2 * q] + v[2 * q + 1]);
      mod = mod + bg;
      const double t = (sD[k * 64 + lane] - mod) * sW[k * 64 + lane];
      const double x = t * t;
      const double dl = x - sC[k * 64 + lane];
      a1[k] += dl;
      a2[k] = fma(dl, dl, a2[k]);
      // one exp either way: a new minimum rescales the sum, anything else joins it
      const double e = dev::exp_neg(fabs(x - mn[k]) * 0.5);
      const bool lower = x < mn[k];
      ls[k] = lower ? fma(ls[k], e, 1.0) : ls[k] + e;
      mn[k] = lower ? x : mn[k];
    }
    cur = nxt;
  }
  const size_t npix = (size_t)n * n;
  double *o = part + (size_t)blk * 4 * npix;
#pragma unroll
  for (int k = 0; k < R; ++k)
    if (act && r0 + k < n) {
      const size_t pix = (size_t)(r0 + k) * n + j;
      o[pix] = a1[k];
      o[npix + pix] = a2[k];
      o[2 * npix + pix] = mn[k];
      o[3 * npix + pix] = ls[k];
    }
}

// 6. reduce: the piece's partials into the running state, in block order (nb < 0: the
// piece's blocks as the book kernel counted them; olpe_lik_add merges one block)
__global__ __launch_bounds__(kThreads) void lik_reduce_kernel(
    const unsigned long long *__restrict__ words, int nb, const double *__restrict__ part,
    size_t npix, double *__restrict__ sum) {
  const size_t pix = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (pix >= npix) return;
  if (nb < 0) nb = (int)((words[kWPiece] + kB - 1) / kB);
  double s1 = sum[pix], s2 = sum[npix + pix], m = sum[2 * npix + pix], L = sum[3 * npix + pix];
  int b = 0;
  for (; b + 8 <= nb; b += 8) {               // eight blocks' loads in flight, merged in order
    double p[8][4];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) p[u][q] = part[((size_t)(b + u) * 4 + q) * npix + pix];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s1 += p[u][0];
      s2 += p[u][1];
      lse_merge(m, L, p[u][2], p[u][3]);
    }
  }
  for (; b < nb; ++b) {
    const double *q = part + (size_t)b * 4 * npix + pix;
    s1 += q[0];
    s2 += q[npix];
    lse_merge(m, L, q[2 * npix], q[3 * npix]);
  }
  sum[pix] = s1;
  sum[npix + pix] = s2;
  sum[2 * npix + pix] = m;
  sum[3 * npix + pix] = L;
}

// The planes of olpe.h, and per block of 256 pixels their sums over the pixels that count
// (unmasked, every sum finite) by a fixed tree; the host adds the blocks in order
template <int NSRC>
__global__ __launch_bounds__(kThreads) void lik_finalize_kernel(
    const double2 *__restrict__ DE, const double *__restrict__ sum,
    const double *__restrict__ cimg, const double *__restrict__ best,
    const double *__restrict__ vec, int have_vec, double nused, int n, int bkgd_mode,
    double *__restrict__ planes, FinPart *__restrict__ fin) {
  __shared__ double s_v[7][kThreads];
  __shared__ int s_c[3][kThreads];
  const int t = threadIdx.x;
  const size_t npix = (size_t)n * n;
  const size_t pix = (size_t)blockIdx.x * kThreads + t;
  double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int c[3] = {0, 0, 0};
  if (pix < npix) {
    double d[12 * NSRC + 1];
    const int i = (int)(pix / n), j = (int)(pix - (size_t)i * n);
    const double2 de = DE[pix];
    make_desc<NSRC>(best, bkgd_mode, d);
    const double xb = pixel_dev<NSRC>(d, j, i, de);
    double xa = nan("");
    if (have_vec) {
      make_desc<NSRC>(vec, bkgd_mode, d);
      xa = pixel_dev<NSRC>(d, j, i, de);
    }
    const double s1 = sum[pix], s2 = sum[npix + pix], m = sum[2 * npix + pix],
                 L = sum[3 * npix + pix];
    const double m1 = s1 / nused;
    const double mean = cimg[pix] + m1;
    const double vnum = s2 - s1 * m1;
    const double var = vnum / nused;
    const double lppd = log(L / nused) - m * 0.5;
    const double pw = nused > 1.0 ? vnum / (nused - 1.0) * 0.25 : 0.0;
    const double elpd = lppd - pw;
    const bool masked = de.y == 0.0;
    const bool bad = !(isfinite(s1) && isfinite(s2) && isfinite(m) && isfinite(L) &&
                       isfinite(mean) && isfinite(vnum));
    const bool out = masked || bad;
    planes[pix] = out ? nan("") : mean;
    planes[npix + pix] = out ? nan("") : (var > 0.0 ? sqrt(var) : 0.0);
    planes[2 * npix + pix] = out ? nan("") : lppd;
    planes[3 * npix + pix] = out ? nan("") : pw;
    planes[4 * npix + pix] = out ? nan("") : elpd;
    planes[5 * npix + pix] = out ? nan("") : xb;
    planes[6 * npix + pix] = out ? nan("") : xa;
    if (!masked) {
      c[0] = 1;
      c[1] = bad;
      v[6] = log(de.y) - 0.91893853320467274178;   // log w - log(2 pi) / 2
      if (!bad) {
        c[2] = pw > 0.4;
        v[0] = lppd;
        v[1] = pw;
        v[2] = elpd;
        v[3] = mean;
        v[4] = xb;
        v[5] = have_vec ? xa : 0.0;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 7; ++q) s_v[q][t] = v[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) s_c[q][t] = c[q];
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int q = 0; q < 7; ++q) s_v[q][t] += s_v[q][t + o];
#pragma unroll
      for (int q = 0; q < 3; ++q) s_c[q][t] += s_c[q][t + o];
    }
    __syncthreads();
  }
  if (t == 0)
    fin[blockIdx.x] = FinPart{s_v[0][0], s_v[1][0], s_v[2][0], s_v[3][0], s_v[4][0], s_v[5][0],
                              s_v[6][0], s_c[0][0], s_c[1][0], s_c[2][0]};
}

int tiles_of(const olpe_lik *r) { return ((r->n + 63) / 64) * ((r->n + r->rows - 1) / r->rows); }

template <int NSRC>
int launch_piece_t(olpe_lik *r, hipStream_t st, const RowMap &m, long long s0, int ns) {
  using L = dev::Layout<NSRC>;
  const int nblk = (ns + kB - 1) / kB;
  BlkInfo *info = (BlkInfo *)r->d_info;
  const unsigned pixblocks = (unsigned)((r->npix + kThreads - 1) / kThreads);
  hipLaunchKernelGGL((resid_scan_kernel<L::NP>), dim3(nblk), dim3(kThreads), 0, st, m, s0, ns, info);
  hipLaunchKernelGGL((resid_book_kernel<L::PS>), dim3(1), dim3(kMaxPieceBlocks), 0, st, m, s0, nblk, info,
                     r->d_boff, r->d_words, r->d_pivot, r->d_best);
  hipLaunchKernelGGL((lik_pivot_kernel<NSRC>), dim3(pixblocks), dim3(kThreads), 0, st,
                     r->d_words, 0, r->d_pivot, r->d_DE, r->n, r->bkgd_mode, r->d_cimg);
  hipLaunchKernelGGL((resid_desc_kernel<NSRC>), dim3(nblk), dim3(kThreads), 0, st, m, s0, ns,
                     r->d_boff, r->bkgd_mode, r->d_desc);
  const dim3 grid((unsigned)((nblk + kThreads / 64 - 1) / (kThreads / 64)), (unsigned)tiles_of(r));
  if (r->rows == 4)
    hipLaunchKernelGGL((lik_fold_kernel<NSRC, 4>), grid, dim3(kThreads), 0, st, r->d_desc,
                       r->d_words, r->d_DE, r->d_cimg, r->n, r->d_part);
  else
    hipLaunchKernelGGL((lik_fold_kernel<NSRC, 8>), grid, dim3(kThreads), 0, st, r->d_desc,
                       r->d_words, r->d_DE, r->d_cimg, r->n, r->d_part);
  hipLaunchKernelGGL(lik_reduce_kernel, dim3(pixblocks), dim3(kThreads), 0, st, r->d_words, -1,
                     r->d_part, r->npix, r->d_sum);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

// `count` samples of the map on `st`, a piece at a time (a piece is a whole number of
// blocks, so the order of a pixel's operations does not depend on the piece size)
int launch_fold(olpe_lik *r, hipStream_t st, const RowMap &m, long long count) {
  const long long piece = (long long)r->piece_blocks * kB;
  for (long long s0 = 0; s0 < count; s0 += piece) {
    const int ns = (int)std::min(piece, count - s0);
    const int rc = r->nsrc == 2 ? launch_piece_t<2>(r, st, m, s0, ns)
                                : launch_piece_t<3>(r, st, m, s0, ns);
    if (rc) return rc;
  }
  return OLPE_OK;
}

// the pivot vector at d_pivot -> the plane c, on the object's stream (waited for)
int set_pivot(olpe_lik *r, const double *pivot) {
  HIPCHK(hipMemcpyAsync(r->d_pivot, pivot, (size_t)r->ps * 8, hipMemcpyHostToDevice, r->stream));
  const unsigned pixblocks = (unsigned)((r->npix + kThreads - 1) / kThreads);
  if (r->nsrc == 2)
    hipLaunchKernelGGL((lik_pivot_kernel<2>), dim3(pixblocks), dim3(kThreads), 0, r->stream,
                       r->d_words, 1, r->d_pivot, r->d_DE, r->n, r->bkgd_mode, r->d_cimg);
  else
    hipLaunchKernelGGL((lik_pivot_kernel<3>), dim3(pixblocks), dim3(kThreads), 0, r->stream,
                       r->d_words, 1, r->d_pivot, r->d_DE, r->n, r->bkgd_mode, r->d_cimg);
  HIPCHK(hipGetLastError());
  unsigned long long one = 1;
  HIPCHK(hipMemcpyAsync(r->d_words + kWHavePivot, &one, 8, hipMemcpyHostToDevice, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  return OLPE_OK;
}

int read_words(olpe_lik *r, unsigned long long *w) {
  HIPCHK(hipMemcpy(w, r->d_words, kWords * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

// the empty state: A1 = A2 = L = 0, m = +inf (nothing of the object in flight)
int clear_sums(olpe_lik *r) {
  std::vector<double> z(4 * r->npix, 0.0);
  std::fill(z.begin() + 2 * r->npix, z.begin() + 3 * r->npix, (double)INFINITY);
  HIPCHK(hipMemcpy(r->d_sum, z.data(), 4 * r->npix * 8, hipMemcpyHostToDevice));
  return OLPE_OK;
}

// vec's np parameters at d_vec, on the object's stream
int stage_vec(olpe_lik *r, const double *vec) {
  std::vector<double> v(vec, vec + r->np);
  v.push_back(0.0);                             // the chi^2 column plays no part
  HIPCHK(hipMemcpyAsync(r->d_vec, v.data(), (size_t)r->ps * 8, hipMemcpyHostToDevice, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));      // v goes out of scope
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_lik_create(olpe_ctx *c, const double *pivot, olpe_lik **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (!c) return set_err(OLPE_EINVAL, "NULL context");
  if (pivot && !finite_params(pivot, c->np))
    return set_err(OLPE_EINVAL, "the pivot vector has a non-finite parameter");
  int rows = 8;
  if (const char *e = getenv("OLPE_LIK_ROWS")) {                            // A/B, tests
    rows = atoi(e);
    if (rows != 4 && rows != 8)
      return set_err(OLPE_EINVAL, "OLPE_LIK_ROWS=%s: 4 or 8 rows per tile", e);
  }
  const size_t npix = (size_t)c->n * c->n;
  const size_t per_block = npix * 32;          // a block's partials
  if (per_block > kPartLimit)
    return set_err(OLPE_EINVAL, "a %dx%d frame needs %zu bytes of partial sums per block of %d "
                   "samples; the limit is %zu", c->n, c->n, per_block, kB, kPartLimit);
  const long long tiles = (long long)((c->n + 63) / 64) * ((c->n + rows - 1) / rows);
  if (tiles > 65535)
    return set_err(OLPE_EINVAL, "a %dx%d frame has %lld tiles of 64 x %d pixels; a grid "
                   "takes 65535", c->n, c->n, tiles, rows);
  HIPCHK(hipSetDevice(c->device));
  olpe_lik *r = new olpe_lik;
  r->n = c->n;
  r->nsrc = c->nsrc;
  r->np = c->np;
  r->bkgd_mode = c->bkgd_mode;
  r->ps = c->ps;
  r->rows = rows;
  r->npix = npix;
  r->piece_blocks = (int)std::min<size_t>(kMaxPieceBlocks, std::max<size_t>(1, kPartBudget / per_block));
  const size_t ks = 12 * (size_t)c->nsrc + 1, pb = (size_t)r->piece_blocks;
  const size_t finblocks = (npix + kThreads - 1) / kThreads;
  int rc = fold_open(r, c->device);
  if (!rc) rc = alloc((void **)&r->d_DE, npix * sizeof(double2), "the cutout");
  if (!rc) rc = alloc((void **)&r->d_sum, 4 * npix * 8, "the pixel state");
  if (!rc) rc = alloc((void **)&r->d_cimg, npix * 8, "the pivot's deviance");
  if (!rc) rc = alloc((void **)&r->d_pivot, (size_t)r->ps * 8, "the pivot vector");
  if (!rc) rc = alloc((void **)&r->d_best, (size_t)r->ps * 8, "the best row");
  if (!rc) rc = alloc((void **)&r->d_vec, (size_t)r->ps * 8, "the point vector");
  if (!rc) rc = alloc((void **)&r->d_words, kWords * 8, "the counters");
  if (!rc) rc = alloc(&r->d_info, pb * sizeof(BlkInfo), "the block table");
  if (!rc) rc = alloc((void **)&r->d_boff, pb * sizeof(int), "the block offsets");
  if (!rc) rc = alloc((void **)&r->d_desc, pb * kB * ks * 8, "the sample descriptors");
  if (!rc) rc = alloc((void **)&r->d_part, pb * per_block, "the partial sums");
  if (!rc) rc = alloc((void **)&r->d_planes, OLPE_LIK_PLANES * npix * 8, "the planes");
  if (!rc) rc = alloc(&r->d_fin, finblocks * sizeof(FinPart), "the finalize partials");
  // the cutout behind whatever the context's stream still has in flight
  if (!rc && (hipStreamSynchronize(olpe_main(c)) != hipSuccess ||
              hipMemcpy(r->d_DE, c->d_DE, npix * sizeof(double2), hipMemcpyDeviceToDevice) != hipSuccess ||
              hipMemset(r->d_cimg, 0, npix * 8) != hipSuccess ||
              hipMemset(r->d_pivot, 0, (size_t)r->ps * 8) != hipSuccess ||
              hipMemset(r->d_best, 0, (size_t)r->ps * 8) != hipSuccess ||
              hipMemset(r->d_vec, 0, (size_t)r->ps * 8) != hipSuccess ||
              hipMemset(r->d_words, 0, kWords * 8) != hipSuccess))
    rc = set_err(OLPE_EHIP, "cutout copy failed");
  if (!rc) rc = clear_sums(r);
  if (!rc && pivot) {
    std::vector<double> pv(pivot, pivot + c->np);
    pv.push_back(0.0);                          // the chi^2 column plays no part
    rc = set_pivot(r, pv.data());
    r->explicit_pivot = true;
  }
  if (rc) {
    olpe_lik_destroy(r);
    return rc;
  }
  *out = r;
  return OLPE_OK;
}

void olpe_lik_destroy(olpe_lik *r) {
  if (!r) return;
  fold_close(r, {r->d_DE, r->d_sum, r->d_cimg, r->d_pivot, r->d_best, r->d_vec, r->d_words,
                 r->d_info, r->d_boff, r->d_desc, r->d_part, r->d_planes, r->d_fin, r->d_stage});
  delete r;
}

int olpe_lik_fold_ctx(olpe_lik *r, olpe_ctx *c, int row_step, int walker_step) {
  if (!r || !c) return set_err(OLPE_EINVAL, "NULL argument");
  if (row_step <= 0 || walker_step <= 0)
    return set_err(OLPE_EINVAL, "row_step %d, walker_step %d: both must be > 0", row_step,
                   walker_step);
  if (c->device != r->device || c->n != r->n || c->nsrc != r->nsrc || c->bkgd_mode != r->bkgd_mode)
    return set_err(OLPE_EINVAL, "context of device %d, side %d, %d sources, bkgd_mode %d; this "
                   "object of device %d, side %d, %d sources, bkgd_mode %d", c->device, c->n,
                   c->nsrc, c->bkgd_mode, r->device, r->n, r->nsrc, r->bkgd_mode);
  int rc;
  if ((rc = fold_check(r, c))) return rc;
  HIPCHK(hipSetDevice(r->device));
  // rows 0, row_step, ... of walkers 0, walker_step, ... of the chain [W][nrec][PS],
  // walker-major: indexing only
  const long long nr = (c->chain_rows + row_step - 1) / row_step;
  const long long nw = ((long long)c->W + walker_step - 1) / walker_step;
  const RowMap m{c->d_chain, nr, (long long)walker_step * c->chain_rows * c->ps,
                 (long long)row_step * c->ps};
  return fold_run(r, c, nr > 0 && nw > 0,
                  [&](hipStream_t s) { return launch_fold(r, s, m, nr * nw); });
}

int olpe_lik_fold_rows(olpe_lik *r, const double *rows, long long nsamples) {
  if (!r) return set_err(OLPE_EINVAL, "NULL argument");
  if (nsamples < 0 || (nsamples > 0 && !rows))
    return set_err(OLPE_EINVAL, "%lld samples at %p", nsamples, (const void *)rows);
  if (nsamples == 0) return OLPE_OK;
  HIPCHK(hipSetDevice(r->device));
  const long long piece = (long long)r->piece_blocks * kB;
  int rc;
  if (!r->d_stage &&
      (rc = alloc((void **)&r->d_stage, (size_t)piece * r->ps * 8, "the row upload")))
    return rc;
  if ((rc = wait_pending(r))) return rc;
  for (long long s0 = 0; s0 < nsamples; s0 += piece) {
    const long long ns = std::min(piece, nsamples - s0);
    HIPCHK(hipMemcpyAsync(r->d_stage, rows + (size_t)s0 * r->ps, (size_t)ns * r->ps * 8,
                          hipMemcpyHostToDevice, r->stream));
    const RowMap m{r->d_stage, ns, 0, (long long)r->ps};
    if ((rc = launch_fold(r, r->stream, m, ns))) return rc;
    HIPCHK(hipStreamSynchronize(r->stream));   // d_stage is reused
  }
  return OLPE_OK;
}

int olpe_lik_get(olpe_lik *r, long long *n, long long *n_bad, double *pivot, double *a1,
                 double *a2, double *m, double *l, double *best) {
  if (!r) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(r->device));
  int rc;
  if ((rc = drain(r))) return rc;
  unsigned long long w[kWords];
  if ((rc = read_words(r, w))) return rc;
  if (n) *n = (long long)w[kWUsed];
  if (n_bad) *n_bad = (long long)w[kWBad];
  if (pivot) {
    if (w[kWHavePivot]) HIPCHK(hipMemcpy(pivot, r->d_pivot, (size_t)r->ps * 8, hipMemcpyDeviceToHost));
    else for (int k = 0; k < r->ps; ++k) pivot[k] = nan("");
  }
  double *dst[4] = {a1, a2, m, l};
  for (int q = 0; q < 4; ++q)
    if (dst[q])
      HIPCHK(hipMemcpy(dst[q], r->d_sum + q * r->npix, r->npix * 8, hipMemcpyDeviceToHost));
  if (best) {
    if (w[kWHaveBest]) HIPCHK(hipMemcpy(best, r->d_best, (size_t)r->ps * 8, hipMemcpyDeviceToHost));
    else for (int k = 0; k < r->ps; ++k) best[k] = nan("");
  }
  return OLPE_OK;
}

int olpe_lik_add(olpe_lik *r, long long n, long long n_bad, const double *pivot,
                 const double *a1, const double *a2, const double *m, const double *l,
                 const double *best) {
  if (!r || !pivot || !a1 || !a2 || !m || !l || !best)
    return set_err(OLPE_EINVAL, "NULL argument");
  if (n < 0 || n_bad < 0) return set_err(OLPE_EINVAL, "n %lld, n_bad %lld", n, n_bad);
  HIPCHK(hipSetDevice(r->device));
  int rc;
  if ((rc = drain(r))) return rc;
  unsigned long long w[kWords];
  if ((rc = read_words(r, w))) return rc;
  if (n > 0) {
    std::vector<double> cur((size_t)r->ps);
    HIPCHK(hipMemcpy(cur.data(), r->d_pivot, (size_t)r->ps * 8, hipMemcpyDeviceToHost));
    if (w[kWUsed] == 0) {
      // empty: the incoming pivot becomes this object's
      if (!finite_params(pivot, r->ps - 1))
        return set_err(OLPE_EINVAL, "the incoming pivot has a non-finite parameter");
      if (!w[kWHavePivot] || memcmp(cur.data(), pivot, (size_t)(r->ps - 1) * 8)) {
        if ((rc = set_pivot(r, pivot))) return rc;
        r->explicit_pivot = false;
      }
    } else if (memcmp(cur.data(), pivot, (size_t)(r->ps - 1) * 8)) {
      return set_err(OLPE_EINVAL, "the pivots differ: sums about different planes do not add");
    }
    // the incoming state as one block of partials: the reduce kernel's own merge
    const double *src[4] = {a1, a2, m, l};
    for (int q = 0; q < 4; ++q)
      HIPCHK(hipMemcpyAsync(r->d_part + q * r->npix, src[q], r->npix * 8, hipMemcpyHostToDevice,
                            r->stream));
    hipLaunchKernelGGL(lik_reduce_kernel, dim3((unsigned)((r->npix + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, r->stream, r->d_words, 1, r->d_part, r->npix, r->d_sum);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(r->stream));
    // this object's folds come first: the incoming best wins only if strictly smaller
    const double chi = best[r->ps - 1];
    if (chi == chi) {
      double mine = 0.0;
      if (w[kWHaveBest])
        HIPCHK(hipMemcpy(&mine, r->d_best + r->ps - 1, 8, hipMemcpyDeviceToHost));
      if (!w[kWHaveBest] || chi < mine) {
        HIPCHK(hipMemcpy(r->d_best, best, (size_t)r->ps * 8, hipMemcpyHostToDevice));
        w[kWHaveBest] = 1;
      }
    }
  }
  w[kWUsed] += (unsigned long long)n;
  w[kWBad] += (unsigned long long)n_bad;
  HIPCHK(hipMemcpy(r->d_words + kWUsed, &w[kWUsed], 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r->d_words + kWBad, &w[kWBad], 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r->d_words + kWHaveBest, &w[kWHaveBest], 8, hipMemcpyHostToDevice));
  return OLPE_OK;
}

int olpe_lik_reset(olpe_lik *r) {
  if (!r) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(r->device));
  int rc;
  if ((rc = drain(r))) return rc;
  unsigned long long w[kWords] = {};
  w[kWHavePivot] = r->explicit_pivot;          // a pivot given at create stays
  if ((rc = clear_sums(r))) return rc;
  HIPCHK(hipMemcpy(r->d_words, w, kWords * 8, hipMemcpyHostToDevice));
  fold_forget(r);
  return OLPE_OK;
}

int olpe_lik_point(olpe_lik *r, const double *vec, double *plane) {
  if (!r || !vec || !plane) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(r->device));
  int rc;
  if ((rc = drain(r))) return rc;
  if ((rc = stage_vec(r, vec))) return rc;
  const unsigned nb = (unsigned)((r->npix + kThreads - 1) / kThreads);
  // d_planes' last plane: finalize writes it anew
  double *img = r->d_planes + (size_t)(OLPE_LIK_PLANES - 1) * r->npix;
  if (r->nsrc == 2)
    hipLaunchKernelGGL((lik_point_kernel<2>), dim3(nb), dim3(kThreads), 0, r->stream, r->d_vec,
                       r->d_DE, r->n, r->bkgd_mode, img);
  else
    hipLaunchKernelGGL((lik_point_kernel<3>), dim3(nb), dim3(kThreads), 0, r->stream, r->d_vec,
                       r->d_DE, r->n, r->bkgd_mode, img);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(plane, img, r->npix * 8, hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  return OLPE_OK;
}

int olpe_lik_finalize(olpe_lik *r, const double *theta_hat, double *planes, double *scalars) {
  if (!r || !planes || !scalars) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(r->device));
  int rc;
  if ((rc = drain(r))) return rc;
  unsigned long long w[kWords];
  if ((rc = read_words(r, w))) return rc;
  if (w[kWUsed] == 0)
    return set_err(OLPE_ESTATE, "no usable sample folded (%llu unusable)", w[kWBad]);
  if (!w[kWHaveBest])
    return set_err(OLPE_ESTATE, "the chi^2 column of all %llu usable samples is NaN: no best "
                   "sample", w[kWUsed]);
  if (theta_hat && (rc = stage_vec(r, theta_hat))) return rc;
  const unsigned nb = (unsigned)((r->npix + kThreads - 1) / kThreads);
  FinPart *fin = (FinPart *)r->d_fin;
  const int have = theta_hat != nullptr;
  if (r->nsrc == 2)
    hipLaunchKernelGGL((lik_finalize_kernel<2>), dim3(nb), dim3(kThreads), 0, r->stream, r->d_DE,
                       r->d_sum, r->d_cimg, r->d_best, r->d_vec, have, (double)w[kWUsed], r->n,
                       r->bkgd_mode, r->d_planes, fin);
  else
    hipLaunchKernelGGL((lik_finalize_kernel<3>), dim3(nb), dim3(kThreads), 0, r->stream, r->d_DE,
                       r->d_sum, r->d_cimg, r->d_best, r->d_vec, have, (double)w[kWUsed], r->n,
                       r->bkgd_mode, r->d_planes, fin);
  HIPCHK(hipGetLastError());
  std::vector<FinPart> hf(nb);
  HIPCHK(hipMemcpyAsync(planes, r->d_planes, OLPE_LIK_PLANES * r->npix * 8,
                        hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipMemcpyAsync(hf.data(), fin, nb * sizeof(FinPart), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  FinPart t{};
  for (const FinPart &f : hf) {                 // in block order
    t.lppd += f.lppd;
    t.pwaic += f.pwaic;
    t.elpd += f.elpd;
    t.mean += f.mean;
    t.best += f.best;
    t.at += f.at;
    t.lognorm += f.lognorm;
    t.cnt += f.cnt;
    t.poisoned += f.poisoned;
    t.high += f.high;
  }
  // var_i(elpd_i), ddof 1, over the pixels that count, in pixel order about their mean
  const double N = (double)(t.cnt - t.poisoned);
  const double *elpd = planes + (size_t)OLPE_LIK_PLANE_ELPD * r->npix;
  const double mu = t.elpd / N;
  double ss = 0.0;
  for (size_t i = 0; i < r->npix; ++i)
    if (elpd[i] == elpd[i]) ss += (elpd[i] - mu) * (elpd[i] - mu);
  const double nanv = nan("");
  scalars[OLPE_LIK_USED] = (double)w[kWUsed];
  scalars[OLPE_LIK_BAD] = (double)w[kWBad];
  scalars[OLPE_LIK_PIXELS] = (double)t.cnt;
  scalars[OLPE_LIK_POISONED] = (double)t.poisoned;
  scalars[OLPE_LIK_LPPD] = t.lppd;
  scalars[OLPE_LIK_P_WAIC] = t.pwaic;
  scalars[OLPE_LIK_ELPD_WAIC] = t.elpd;
  scalars[OLPE_LIK_WAIC] = -2.0 * t.elpd;
  scalars[OLPE_LIK_SE_ELPD] = N > 1.0 ? sqrt(N * (ss / (N - 1.0))) : nanv;
  scalars[OLPE_LIK_P_WAIC_HIGH] = (double)t.high;
  scalars[OLPE_LIK_MEAN_DEVIANCE] = t.mean;
  scalars[OLPE_LIK_REDUCED] = N > (double)r->np ? t.mean / (N - (double)r->np) : nanv;
  scalars[OLPE_LIK_DEVIANCE_BEST] = t.best;
  scalars[OLPE_LIK_DEVIANCE_AT] = have ? t.at : nanv;
  scalars[OLPE_LIK_P_D] = have ? t.mean - t.at : nanv;
  scalars[OLPE_LIK_DIC] = have ? t.at + 2.0 * (t.mean - t.at) : nanv;
  scalars[OLPE_LIK_LOG_NORM] = t.lognorm;
  return OLPE_OK;
}

}  // extern "C"
