// olpe_resid.hip -- the posterior's model and residual images, folded on the device: the
// picture the reference's README opens with (data, model, residual), taken over the whole
// ensemble instead of one vector.  Every sample's model is build_analytical_model
// (apf_step2.py:106-124; 3body/apf_step2_3body.py:106-125) in the EXACT operation order,
// whatever the context's eval mode.
//
// An olpe_resid copies a context's staged cutout and is independent of it afterwards.  It
// keeps, per pixel, the shifted sums over the folded samples s with model M_s and a pivot
// image R (the model of a pivot vector):  S1 = sum (M_s - R),  S2 = sum (M_s - R)^2.
// A piece of at most kMaxPieceBlocks * kB samples goes through six launches:
//   1. scan     per block of kB rows: usable rows (every parameter finite), unusable ones,
//               the first usable row, the smallest chi^2 (NaN never wins) and its row;
//   2. book     one workgroup over the blocks: compact offsets, the counts, the best row so
//               far (strictly smaller wins: the earliest on a tie), and the pivot (the
//               first usable row ever folded, unless the caller gave one);
//   3. pivot    the pivot's model image, only when step 2 took a pivot;
//   4. desc     a thread per row: the sample's Gaussians (make_trig / make_coef /
//               make_model) at its compact position, so unusable rows leave no trace in
//               the order of the sums;
//   5. fold     the hot path.  A wave owns a tile of 64 columns x R rows and a block of kB
//               compacted samples: 2R accumulators in registers, the tile of R in LDS, the
//               sample's descriptor prefetched one ahead (a lane per double, read out with
//               v_readlane), sweep_exact's per-pixel expression, and the block's (S1, S2)
//               of the tile to a partials array;
//   6. reduce   a thread per pixel adds the partials to the running sums in block order.
// No floating-point atomics; a pixel's sums take the same additions in the same order for
// any grid, CU count or tile height.  DESIGN.md §7d has the layout and the measurements.
// Steps 1, 2 and 4, the row map and the per-pixel model are olpe_samples.h's, shared with
// olpe_lik.hip.
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

// The sampler's device functions, by #include only.  In a namespace of this unit's: the
// header's __constant__ tables have external linkage and olpe.hip's object defines them.
namespace olpe_resid_dev {
#include "olpe_device.h"
}
namespace dev = olpe_resid_dev::olpe;

using namespace olpe;

// scan, book, desc and the per-pixel model, shared with olpe_lik.hip
#include "olpe_samples.h"

struct olpe_resid : FoldBase {
  int n = 0, nsrc = 2, bkgd_mode = 0, ps = 17;
  int rows = 16;                // tile height of the fold kernel (8 or 16)
  int piece_blocks = 0;         // blocks of kB samples per piece
  size_t npix = 0;
  bool explicit_pivot = false;  // the pivot came with olpe_resid_create
  double2 *d_DE = nullptr;      // [npix] the context's staged cutout
  double *d_sum = nullptr;      // [2][npix] S1, S2
  double *d_pivimg = nullptr;   // [npix] R
  double *d_pivot = nullptr;    // [ps]
  double *d_best = nullptr;     // [ps]
  unsigned long long *d_words = nullptr;  // [kWords]
  void *d_info = nullptr;       // [piece_blocks] BlkInfo
  int *d_boff = nullptr;        // [piece_blocks] compact offset of each block
  double *d_desc = nullptr;     // [piece_blocks * kB][6 G + 1]
  double *d_part = nullptr;     // [piece_blocks][2][npix]
  double *d_planes = nullptr;   // [OLPE_RESID_PLANES][npix]
  void *d_fin = nullptr;        // [ceil(npix / 256)] FinPart
  double *d_stage = nullptr;    // upload staging of fold_rows (allocated on first use)
};

namespace {

struct FinPart {
  double sum4, sum6, max4;
  int cnt, idx;
};

// 3. pivot: R = the model of the pivot vector, when the book kernel took one (or `force`)
template <int NSRC>
__global__ __launch_bounds__(kThreads) void resid_pivot_kernel(
    const unsigned long long *__restrict__ words, int force, const double *__restrict__ pivot,
    int n, int bkgd_mode, double *__restrict__ img) {
  if (!force && !words[kWPivotNew]) return;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= n * n) return;
  double d[12 * NSRC + 1];
  make_desc<NSRC>(pivot, bkgd_mode, d);
  const int i = pix / n, j = pix - i * n;
  img[pix] = pixel_model<NSRC>(d, (double)j, (double)i);
}

// 5. fold: workgroup (x, y) = tile y, blocks 4 x .. 4 x + 3 of the piece, a wave each.
// Lanes beyond column n - 1 compute the last column, a tile's rows beyond n - 1 are
// computed like the others (no branch in the row loop); neither is stored.
// part[block][2][npix].
template <int NSRC, int R>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void resid_fold_kernel(const double *__restrict__ desc,
                       const unsigned long long *__restrict__ words,
                       const double *__restrict__ pivimg, int n, double *__restrict__ part) {
  constexpr int G = 2 * NSRC, KS = 6 * G + 1;
  static_assert(KS <= 64, "a lane per double of the descriptor");
  __shared__ double piv[R * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tx = (n + 63) >> 6;
  const int trow = blockIdx.y / tx, tcol = blockIdx.y - trow * tx;
  const int j = tcol * 64 + lane, r0 = trow * R;
  const bool act = j < n;
  const int jj = act ? j : n - 1;
  for (int k = wave; k < R; k += kThreads / 64)
    piv[k * 64 + lane] = r0 + k < n ? pivimg[(size_t)(r0 + k) * n + jj] : 0.0;
  __syncthreads();
  const long long cnt = (long long)words[kWPiece];
  const long long blk = (long long)blockIdx.x * (kThreads / 64) + wave;
  if (blk * kB >= cnt) return;
  const int ns = (int)(cnt - blk * kB < kB ? cnt - blk * kB : kB);
  const double *d = desc + (size_t)blk * kB * KS + (lane < KS ? lane : 0);
  const double xj = (double)jj;
  double a1[R], a2[R];
#pragma unroll
  for (int k = 0; k < R; ++k) a1[k] = a2[k] = 0.0;
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
      const double dl = mod - piv[k * 64 + lane];
      a1[k] += dl;
      a2[k] = fma(dl, dl, a2[k]);
    }
    cur = nxt;
  }
  const size_t npix = (size_t)n * n;
  double *o = part + (size_t)blk * 2 * npix;
#pragma unroll
  for (int k = 0; k < R; ++k)
    if (act && r0 + k < n) {
      o[(size_t)(r0 + k) * n + j] = a1[k];
      o[npix + (size_t)(r0 + k) * n + j] = a2[k];
    }
}

// 6. reduce: the piece's partials into the running sums, in block order
__global__ __launch_bounds__(kThreads) void resid_reduce_kernel(
    const unsigned long long *__restrict__ words, const double *__restrict__ part, size_t npix,
    double *__restrict__ sum) {
  const size_t pix = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (pix >= npix) return;
  const int nb = (int)((words[kWPiece] + kB - 1) / kB);
  double s1 = sum[pix], s2 = sum[npix + pix];
  int b = 0;
  for (; b + 8 <= nb; b += 8) {               // eight blocks' loads in flight, added in order
    double p1[8], p2[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      p1[u] = part[(size_t)(b + u) * 2 * npix + pix];
      p2[u] = part[(size_t)(b + u) * 2 * npix + npix + pix];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s1 += p1[u];
      s2 += p2[u];
    }
  }
  for (; b < nb; ++b) {
    s1 += part[(size_t)b * 2 * npix + pix];
    s2 += part[(size_t)b * 2 * npix + npix + pix];
  }
  sum[pix] = s1;
  sum[npix + pix] = s2;
}

// The planes of olpe.h, and per block of 256 pixels the sums, the unmasked count and the
// largest |plane 4| (the lowest pixel on a tie), by a fixed tree; the host adds the blocks
template <int NSRC>
__global__ __launch_bounds__(kThreads) void resid_finalize_kernel(
    const double2 *__restrict__ DE, const double *__restrict__ sum,
    const double *__restrict__ pivimg, const double *__restrict__ best, double nused, int n,
    int bkgd_mode, double *__restrict__ planes, FinPart *__restrict__ fin) {
  __shared__ double s_4[kThreads], s_6[kThreads], s_m[kThreads];
  __shared__ int s_c[kThreads], s_i[kThreads];
  const int t = threadIdx.x;
  const size_t npix = (size_t)n * n;
  const size_t pix = (size_t)blockIdx.x * kThreads + t;
  double q4 = 0.0, q6 = 0.0, m4 = -1.0;
  int cnt = 0, idx = INT_MAX;
  if (pix < npix) {
    double d[12 * NSRC + 1];
    make_desc<NSRC>(best, bkgd_mode, d);
    const int i = (int)(pix / n), j = (int)(pix - (size_t)i * n);
    const double s1 = sum[pix], s2 = sum[npix + pix];
    const double m1 = s1 / nused;
    const double mean = pivimg[pix] + m1;
    const double var = (s2 - s1 * m1) / nused;
    const double mb = pixel_model<NSRC>(d, (double)j, (double)i);
    const double2 de = DE[pix];
    const bool masked = de.y == 0.0;
    const double r3 = de.x - mb, r5 = de.x - mean;
    const double r4 = r3 * de.y, r6 = r5 * de.y;
    planes[pix] = mean;
    planes[npix + pix] = var > 0.0 ? sqrt(var) : 0.0;
    planes[2 * npix + pix] = mb;
    planes[3 * npix + pix] = masked ? nan("") : r3;
    planes[4 * npix + pix] = masked ? nan("") : r4;
    planes[5 * npix + pix] = masked ? nan("") : r5;
    planes[6 * npix + pix] = masked ? nan("") : r6;
    if (!masked) {
      q4 = r4 * r4;
      q6 = r6 * r6;
      cnt = 1;
      if (fabs(r4) >= 0.0) {   // not NaN
        m4 = fabs(r4);
        idx = (int)pix;
      }
    }
  }
  s_4[t] = q4;
  s_6[t] = q6;
  s_m[t] = m4;
  s_c[t] = cnt;
  s_i[t] = idx;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
      s_4[t] += s_4[t + o];
      s_6[t] += s_6[t + o];
      s_c[t] += s_c[t + o];
      if (s_m[t + o] > s_m[t] || (s_m[t + o] == s_m[t] && s_i[t + o] < s_i[t])) {
        s_m[t] = s_m[t + o];
        s_i[t] = s_i[t + o];
      }
    }
    __syncthreads();
  }
  if (t == 0) fin[blockIdx.x] = FinPart{s_4[0], s_6[0], s_m[0], s_c[0], s_i[0]};
}

int tiles_of(const olpe_resid *r) { return ((r->n + 63) / 64) * ((r->n + r->rows - 1) / r->rows); }

template <int NSRC>
int launch_piece_t(olpe_resid *r, hipStream_t st, const RowMap &m, long long s0, int ns) {
  using L = dev::Layout<NSRC>;
  const int nblk = (ns + kB - 1) / kB;
  BlkInfo *info = (BlkInfo *)r->d_info;
  const unsigned pixblocks = (unsigned)((r->npix + kThreads - 1) / kThreads);
  hipLaunchKernelGGL((resid_scan_kernel<L::NP>), dim3(nblk), dim3(kThreads), 0, st, m, s0, ns, info);
  hipLaunchKernelGGL((resid_book_kernel<L::PS>), dim3(1), dim3(kMaxPieceBlocks), 0, st, m, s0, nblk, info,
                     r->d_boff, r->d_words, r->d_pivot, r->d_best);
  hipLaunchKernelGGL((resid_pivot_kernel<NSRC>), dim3(pixblocks), dim3(kThreads), 0, st,
                     r->d_words, 0, r->d_pivot, r->n, r->bkgd_mode, r->d_pivimg);
  hipLaunchKernelGGL((resid_desc_kernel<NSRC>), dim3(nblk), dim3(kThreads), 0, st, m, s0, ns,
                     r->d_boff, r->bkgd_mode, r->d_desc);
  const dim3 grid((unsigned)((nblk + kThreads / 64 - 1) / (kThreads / 64)), (unsigned)tiles_of(r));
  if (r->rows == 8)
    hipLaunchKernelGGL((resid_fold_kernel<NSRC, 8>), grid, dim3(kThreads), 0, st, r->d_desc,
                       r->d_words, r->d_pivimg, r->n, r->d_part);
  else
    hipLaunchKernelGGL((resid_fold_kernel<NSRC, 16>), grid, dim3(kThreads), 0, st, r->d_desc,
                       r->d_words, r->d_pivimg, r->n, r->d_part);
  hipLaunchKernelGGL(resid_reduce_kernel, dim3(pixblocks), dim3(kThreads), 0, st, r->d_words,
                     r->d_part, r->npix, r->d_sum);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

// `count` samples of the map on `st`, a piece at a time (a piece is a whole number of
// blocks, so the order of a pixel's additions does not depend on the piece size)
int launch_fold(olpe_resid *r, hipStream_t st, const RowMap &m, long long count) {
  const long long piece = (long long)r->piece_blocks * kB;
  for (long long s0 = 0; s0 < count; s0 += piece) {
    const int ns = (int)std::min(piece, count - s0);
    const int rc = r->nsrc == 2 ? launch_piece_t<2>(r, st, m, s0, ns)
                                : launch_piece_t<3>(r, st, m, s0, ns);
    if (rc) return rc;
  }
  return OLPE_OK;
}

// the pivot vector at d_pivot -> its image, on the object's stream (waited for)
int set_pivot(olpe_resid *r, const double *pivot) {
  HIPCHK(hipMemcpyAsync(r->d_pivot, pivot, (size_t)r->ps * 8, hipMemcpyHostToDevice, r->stream));
  const unsigned pixblocks = (unsigned)((r->npix + kThreads - 1) / kThreads);
  if (r->nsrc == 2)
    hipLaunchKernelGGL((resid_pivot_kernel<2>), dim3(pixblocks), dim3(kThreads), 0, r->stream,
                       r->d_words, 1, r->d_pivot, r->n, r->bkgd_mode, r->d_pivimg);
  else
    hipLaunchKernelGGL((resid_pivot_kernel<3>), dim3(pixblocks), dim3(kThreads), 0, r->stream,
                       r->d_words, 1, r->d_pivot, r->n, r->bkgd_mode, r->d_pivimg);
  HIPCHK(hipGetLastError());
  unsigned long long one = 1;
  HIPCHK(hipMemcpyAsync(r->d_words + kWHavePivot, &one, 8, hipMemcpyHostToDevice, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  return OLPE_OK;
}

int read_words(olpe_resid *r, unsigned long long *w) {
  HIPCHK(hipMemcpy(w, r->d_words, kWords * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_resid_create(olpe_ctx *c, const double *pivot, olpe_resid **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (!c) return set_err(OLPE_EINVAL, "NULL context");
  if (pivot && !finite_params(pivot, c->np))
    return set_err(OLPE_EINVAL, "the pivot vector has a non-finite parameter");
  int rows = 16;
  if (const char *e = getenv("OLPE_RESID_ROWS")) {                          // A/B, tests
    rows = atoi(e);
    if (rows != 8 && rows != 16)
      return set_err(OLPE_EINVAL, "OLPE_RESID_ROWS=%s: 8 or 16 rows per tile", e);
  }
  const size_t npix = (size_t)c->n * c->n;
  const size_t per_block = npix * 16;          // a block's partials
  if (per_block > kPartLimit)
    return set_err(OLPE_EINVAL, "a %dx%d frame needs %zu bytes of partial sums per block of %d "
                   "samples; the limit is %zu", c->n, c->n, per_block, kB, kPartLimit);
  const long long tiles = (long long)((c->n + 63) / 64) * ((c->n + rows - 1) / rows);
  if (tiles > 65535)
    return set_err(OLPE_EINVAL, "a %dx%d frame has %lld tiles of 64 x %d pixels; a grid "
                   "takes 65535", c->n, c->n, tiles, rows);
  HIPCHK(hipSetDevice(c->device));
  olpe_resid *r = new olpe_resid;
  r->n = c->n;
  r->nsrc = c->nsrc;
  r->bkgd_mode = c->bkgd_mode;
  r->ps = c->ps;
  r->rows = rows;
  r->npix = npix;
  r->piece_blocks = (int)std::min<size_t>(kMaxPieceBlocks, std::max<size_t>(1, kPartBudget / per_block));
  const size_t ks = 12 * (size_t)c->nsrc + 1, pb = (size_t)r->piece_blocks;
  const size_t finblocks = (npix + kThreads - 1) / kThreads;
  int rc = fold_open(r, c->device);
  if (!rc) rc = alloc((void **)&r->d_DE, npix * sizeof(double2), "the cutout");
  if (!rc) rc = alloc((void **)&r->d_sum, 2 * npix * 8, "the shifted sums");
  if (!rc) rc = alloc((void **)&r->d_pivimg, npix * 8, "the pivot image");
  if (!rc) rc = alloc((void **)&r->d_pivot, (size_t)r->ps * 8, "the pivot vector");
  if (!rc) rc = alloc((void **)&r->d_best, (size_t)r->ps * 8, "the best row");
  if (!rc) rc = alloc((void **)&r->d_words, kWords * 8, "the counters");
  if (!rc) rc = alloc(&r->d_info, pb * sizeof(BlkInfo), "the block table");
  if (!rc) rc = alloc((void **)&r->d_boff, pb * sizeof(int), "the block offsets");
  if (!rc) rc = alloc((void **)&r->d_desc, pb * kB * ks * 8, "the sample descriptors");
  if (!rc) rc = alloc((void **)&r->d_part, pb * per_block, "the partial sums");
  if (!rc) rc = alloc((void **)&r->d_planes, OLPE_RESID_PLANES * npix * 8, "the planes");
  if (!rc) rc = alloc(&r->d_fin, finblocks * sizeof(FinPart), "the finalize partials");
  // the cutout behind whatever the context's stream still has in flight
  if (!rc && (hipStreamSynchronize(olpe_main(c)) != hipSuccess ||
              hipMemcpy(r->d_DE, c->d_DE, npix * sizeof(double2), hipMemcpyDeviceToDevice) != hipSuccess ||
              hipMemset(r->d_sum, 0, 2 * npix * 8) != hipSuccess ||
              hipMemset(r->d_pivimg, 0, npix * 8) != hipSuccess ||
              hipMemset(r->d_pivot, 0, (size_t)r->ps * 8) != hipSuccess ||
              hipMemset(r->d_best, 0, (size_t)r->ps * 8) != hipSuccess ||
              hipMemset(r->d_words, 0, kWords * 8) != hipSuccess))
    rc = set_err(OLPE_EHIP, "cutout copy failed");
  if (!rc && pivot) {
    std::vector<double> pv(pivot, pivot + c->np);
    pv.push_back(0.0);                          // the chi^2 column plays no part
    rc = set_pivot(r, pv.data());
    r->explicit_pivot = true;
  }
  if (rc) {
    olpe_resid_destroy(r);
    return rc;
  }
  *out = r;
  return OLPE_OK;
}

void olpe_resid_destroy(olpe_resid *r) {
  if (!r) return;
  fold_close(r, {r->d_DE, r->d_sum, r->d_pivimg, r->d_pivot, r->d_best, r->d_words, r->d_info,
                 r->d_boff, r->d_desc, r->d_part, r->d_planes, r->d_fin, r->d_stage});
  delete r;
}

int olpe_resid_fold_ctx(olpe_resid *r, olpe_ctx *c, int row_step, int walker_step) {
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

int olpe_resid_fold_rows(olpe_resid *r, const double *rows, long long nsamples) {
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

int olpe_resid_get(olpe_resid *r, long long *n, long long *n_bad, double *pivot, double *s1,
                   double *s2, double *best) {
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
  if (s1) HIPCHK(hipMemcpy(s1, r->d_sum, r->npix * 8, hipMemcpyDeviceToHost));
  if (s2) HIPCHK(hipMemcpy(s2, r->d_sum + r->npix, r->npix * 8, hipMemcpyDeviceToHost));
  if (best) {
    if (w[kWHaveBest]) HIPCHK(hipMemcpy(best, r->d_best, (size_t)r->ps * 8, hipMemcpyDeviceToHost));
    else for (int k = 0; k < r->ps; ++k) best[k] = nan("");
  }
  return OLPE_OK;
}

int olpe_resid_add(olpe_resid *r, long long n, long long n_bad, const double *pivot,
                   const double *s1, const double *s2, const double *best) {
  if (!r || !pivot || !s1 || !s2 || !best) return set_err(OLPE_EINVAL, "NULL argument");
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
      return set_err(OLPE_EINVAL, "the pivots differ: sums about different images do not add");
    }
    std::vector<double> sum(2 * r->npix);
    HIPCHK(hipMemcpy(sum.data(), r->d_sum, 2 * r->npix * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < r->npix; ++i) {
      sum[i] += s1[i];
      sum[r->npix + i] += s2[i];
    }
    HIPCHK(hipMemcpy(r->d_sum, sum.data(), 2 * r->npix * 8, hipMemcpyHostToDevice));
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

int olpe_resid_reset(olpe_resid *r) {
  if (!r) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(r->device));
  int rc;
  if ((rc = drain(r))) return rc;
  unsigned long long w[kWords] = {};
  w[kWHavePivot] = r->explicit_pivot;          // a pivot given at create stays
  HIPCHK(hipMemset(r->d_sum, 0, 2 * r->npix * 8));
  HIPCHK(hipMemcpy(r->d_words, w, kWords * 8, hipMemcpyHostToDevice));
  fold_forget(r);
  return OLPE_OK;
}

int olpe_resid_finalize(olpe_resid *r, double *planes, double *scalars) {
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
  const unsigned nb = (unsigned)((r->npix + kThreads - 1) / kThreads);
  FinPart *fin = (FinPart *)r->d_fin;
  if (r->nsrc == 2)
    hipLaunchKernelGGL((resid_finalize_kernel<2>), dim3(nb), dim3(kThreads), 0, r->stream, r->d_DE,
                       r->d_sum, r->d_pivimg, r->d_best, (double)w[kWUsed], r->n, r->bkgd_mode,
                       r->d_planes, fin);
  else
    hipLaunchKernelGGL((resid_finalize_kernel<3>), dim3(nb), dim3(kThreads), 0, r->stream, r->d_DE,
                       r->d_sum, r->d_pivimg, r->d_best, (double)w[kWUsed], r->n, r->bkgd_mode,
                       r->d_planes, fin);
  HIPCHK(hipGetLastError());
  std::vector<FinPart> hf(nb);
  double chi = 0.0;
  HIPCHK(hipMemcpyAsync(planes, r->d_planes, OLPE_RESID_PLANES * r->npix * 8,
                        hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipMemcpyAsync(hf.data(), fin, nb * sizeof(FinPart), hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipMemcpyAsync(&chi, r->d_best + r->ps - 1, 8, hipMemcpyDeviceToHost, r->stream));
  HIPCHK(hipStreamSynchronize(r->stream));
  double sum4 = 0.0, sum6 = 0.0, max4 = -1.0;
  long long cnt = 0, idx = -1;
  for (const FinPart &f : hf) {                 // in block order
    sum4 += f.sum4;
    sum6 += f.sum6;
    cnt += f.cnt;
    if (f.idx != INT_MAX && f.max4 > max4) {
      max4 = f.max4;
      idx = f.idx;
    }
  }
  scalars[0] = (double)w[kWUsed];
  scalars[1] = (double)w[kWBad];
  scalars[2] = (double)cnt;
  scalars[3] = chi;
  scalars[4] = sum4;
  scalars[5] = sum6;
  scalars[6] = idx >= 0 ? max4 : nan("");
  scalars[7] = (double)idx;
  return OLPE_OK;
}

}  // extern "C"
