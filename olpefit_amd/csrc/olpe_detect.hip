// olpe_detect.hip -- the companion detection map of a fit, folded on the device: at every
// candidate position c of a lattice over the frame, the matched filter of the residual with
// the sample's own unit PSF, i.e. the maximum-likelihood amplitude of one more source of the
// shared shape (apf_step2.py:78-103) with its sigma, taken over the whole ensemble so that
// the PSF's posterior scatter enters the detection sigma.  Per sample theta, pixels i,
//   psi(u, v) = (1 - q) g1(u, v) + q g2(u - dx, v - dy),  g_k = exp(-((a_k u^2) + (b_k u) v + c_k v^2))
//   z_i = w_i (D_i - M_i(theta)),  w_i = (1 / err_i)^2 (0 where masked),  K_i(c) = psi(x_i - x_c, y_i - y_c)
//   N(c) = sum_i z_i K_i(c),  Q(c) = sum_i w_i K_i(c)^2,  A = N / Q,  sigma_A = 1 / sqrt(Q),  snr = N / sqrt(Q)
// with the model M and the coefficients a, b, c in the EXACT operation order (make_desc,
// pixel_model), whatever the context's eval mode.  This is a score test: the fitted sources
// stay at the sample's values, nothing is refitted.
//
// The lattice is x_c, y_c = j / os, j = 0 .. os (n - 1), os in {1, 2, 4}: G = (os (n - 1) + 1)^2
// candidates.  psi is translation invariant, so a candidate j = os c + p of phase p sees the
// pixels through one table per phase, P_p[d][e] = psi(e - px / os, d - py / os) on the integer
// offsets d, e = -(n - 1) .. n - 1 (the offsets are exact doubles): os^2 problems of the os = 1
// shape.
//
// An olpe_detect copies a context's staged cutout and is independent of it afterwards.  It
// keeps five planes [G] of sums over the folded samples, shifted about the pivot vector's
// planes (A_p, snr_p):  sum (A - A_p), sum (A - A_p)^2, sum sigma_A^2, sum (snr - snr_p),
// sum (snr - snr_p)^2.  A piece of at most piece_blocks * kB samples goes through
//   1. scan, 2. book     olpe_samples.h's, as in olpe_resid.hip;
//   3. pivot             the pivot's planes (steps 6 - 7 on the one vector, then A, sigma,
//                        snr), only when step 2 took a pivot;
//   4. desc, 5. index    the usable rows' models at their compact positions, and the sample
//                        behind each compact position (q, dx, dy are read from the row);
//   6. prep              a thread per element: the sample's z and w planes (zero rows above
//                        and below, so the correlation needs no row test) and its tables;
//   7. corr              the hot path, 2 G n^2 FMAs per sample.  A workgroup takes a sample,
//                        a phase, 64 candidate columns and 2 kR candidate rows, a wave kR of
//                        them with N and Q in registers.  The workgroup walks the table's
//                        rows d through LDS, kD at a time; at row d candidate row cy meets
//                        pixel row d + cy, whose z and w are wave-uniform (scalar loads),
//                        and one LDS read of P feeds 2 kR FMAs.  A candidate's sums run
//                        over the pixels row by row, column by column: the order is fixed by
//                        the definition, not by the grid;
//   8. stats             a thread per candidate and block of kB compacted samples: the five
//                        shifted sums of the block, sample by sample, to a partials array;
//   9. reduce            the partials into the running sums in block order.
// No floating-point atomics.  finalize is host arithmetic on the state (detect.py's
// planes_from_state restates it).  DESIGN.md §7l has the layout and the measurements.
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

// The sampler's device functions, by #include only (see olpe_resid.hip)
namespace olpe_detect_dev {
#include "olpe_device.h"
}
namespace dev = olpe_detect_dev::olpe;

using namespace olpe;

// scan, book, desc and the per-pixel model, shared with olpe_resid.hip and olpe_lik.hip
#include "olpe_samples.h"

struct olpe_detect : FoldBase {
  int n = 0, nsrc = 2, bkgd_mode = 0, ps = 17, os = 1;
  int gs = 0;                   // lattice side os (n - 1) + 1
  int piece_blocks = 0;         // blocks of kB samples per piece
  long long pixels = 0;         // unmasked pixels
  size_t npix = 0, G = 0;
  size_t tabs = 0;              // doubles of one sample's tables: os^2 (2n - 1)^2
  size_t zws = 0;               // double2 of one sample's padded {z, w} plane
  bool explicit_pivot = false;  // the pivot came with olpe_detect_create
  double2 *d_DE = nullptr;      // [npix] the context's staged cutout
  double *d_sum = nullptr;      // [5][G] the shifted sums
  double *d_piv = nullptr;      // [3][G] the pivot's A, sigma_A, snr
  double *d_out = nullptr;      // [3][G] planes of one vector (point, the best row)
  double *d_pivot = nullptr;    // [ps]
  double *d_best = nullptr;     // [ps]
  double *d_vec = nullptr;      // [ps] olpe_detect_point's vector
  unsigned long long *d_words = nullptr;  // [kWords]
  void *d_info = nullptr;       // [piece_blocks] BlkInfo
  int *d_boff = nullptr;        // [piece_blocks] compact offset of each block
  int *d_idx = nullptr;         // [piece_blocks * kB] compact position -> sample of the piece
  double *d_desc = nullptr;     // [piece_blocks * kB][6 G + 1]
  double *d_tab = nullptr;      // [piece_blocks * kB][tabs]
  double2 *d_zw = nullptr;      // [piece_blocks * kB][zws]
  double *d_nq = nullptr;       // [piece_blocks * kB][2][G] N, Q
  double *d_part = nullptr;     // [piece_blocks][5][G]
  double *d_stage = nullptr;    // upload staging of fold_rows (allocated on first use)
};

namespace {

constexpr int kR = 8;           // candidate rows per wave of the correlation
constexpr int kD = 8;           // table rows staged in LDS at a time
constexpr int kCorrWaves = 2;   // waves per workgroup of the correlation
constexpr int kCorrThreads = 64 * kCorrWaves;
constexpr int kPad = kR;        // zero rows above and below a sample's {z, w} plane
constexpr int kMaxSide = 128;   // n + 63 table columns of a tile fit kSegW
constexpr int kSegW = 192;
constexpr int kSums = 5;
constexpr size_t kWorkBudget = 512u << 20;   // bytes of per-sample work buffers a piece aims at

// Which samples a launch of steps 6 - 7 works on.  kPiece: the piece's compacted samples;
// kPivotNew: the vector handed in, in slot 0, if the book kernel took a pivot; kOne: that
// vector, always.
enum { kPiece = 0, kPivotNew = 1, kOne = 2 };
__device__ __forceinline__ int work_count(const unsigned long long *words, int mode) {
  if (mode == kPiece) return (int)words[kWPiece];
  return mode == kOne || words[kWPivotNew] ? 1 : 0;
}

// A, sigma_A^2, snr of one candidate; a candidate no unmasked pixel sees (Q = 0) is NaN
__device__ __forceinline__ void amplitude(double N, double Q, double *A, double *var,
                                          double *snr) {
  if (Q > 0.0) {
    *A = N / Q;
    *var = 1.0 / Q;
    *snr = N / sqrt(Q);
  } else {
    *A = *var = *snr = nan("");
  }
}

// 3. the one vector's model descriptor into slot 0
template <int NSRC>
__global__ __launch_bounds__(64) void detect_rowdesc_kernel(
    const unsigned long long *__restrict__ words, int mode, const double *__restrict__ row,
    int bkgd_mode, double *__restrict__ desc) {
  if (threadIdx.x || !work_count(words, mode)) return;
  make_desc<NSRC>(row, bkgd_mode, desc);
}

// 5. index: resid_desc_kernel's compaction, keeping the sample instead of its model
template <int NP>
__global__ __launch_bounds__(kThreads) void detect_index_kernel(RowMap m, long long s0, int ns,
                                                                const int *__restrict__ boff,
                                                                int *__restrict__ idx) {
  __shared__ int s_w[kThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int s = blockIdx.x * kB + t;
  const double *row = row_of(m, s0 + (s < ns ? s : 0));
  const bool ok = s < ns && usable_row<NP>(row);
  const unsigned long long bal = __ballot(ok);
  if (lane == 0) s_w[wave] = __popcll(bal);
  __syncthreads();
  int pos = boff[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += s_w[w];
  if (ok) idx[pos] = s;
}

// 6. prep: workgroup (x, y) = elements 256 x .. of sample y: first the n^2 pixels' {z, w},
// then the os^2 (2n - 1)^2 table entries
template <int NSRC>
__global__ __launch_bounds__(kThreads) void detect_prep_kernel(
    const unsigned long long *__restrict__ words, int mode, RowMap m, long long s0,
    const int *__restrict__ idx, const double *__restrict__ one,
    const double *__restrict__ desc, const double2 *__restrict__ DE, int n, int os, size_t tabs,
    size_t zws, double *__restrict__ tab, double2 *__restrict__ zw) {
  using L = dev::Layout<NSRC>;
  constexpr int KS = 12 * NSRC + 1;
  const int s = blockIdx.y;
  if (s >= work_count(words, mode)) return;
  const double *d = desc + (size_t)s * KS;
  const size_t npix = (size_t)n * n;
  const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (t < npix) {
    const int i = (int)(t / n), j = (int)(t - (size_t)i * n);
    const double mod = pixel_model<NSRC>(d, (double)j, (double)i);
    const double2 de = DE[t];
    const double w = de.y * de.y;
    zw[(size_t)s * zws + (size_t)(kPad + i) * n + j] = make_double2(w * (de.x - mod), w);
    return;
  }
  const size_t k = t - npix;
  if (k >= tabs) return;
  const double *row = mode == kPiece ? row_of(m, s0 + idx[s]) : one;
  const double q = row[L::RATIO], dx = row[L::DX], dy = row[L::DY];
  const int T = 2 * n - 1;
  const size_t tt = (size_t)T * T;
  const int ph = (int)(k / tt);
  const size_t rem = k - (size_t)ph * tt;
  const int dd = (int)(rem / T), ee = (int)(rem - (size_t)dd * T);
  const int py = ph / os, px = ph - py * os;
  // the offsets are exact: integers minus a multiple of 1 / os
  const double u = (double)(ee - (n - 1)) - (double)px / (double)os;
  const double v = (double)(dd - (n - 1)) - (double)py / (double)os;
  // narrow: Gaussian 1 of the descriptor, wide: Gaussian 0 (make_model's order)
  const double q1 = (d[9] * (u * u) + (d[10] * u) * v) + d[11] * (v * v);
  const double u2 = u - dx, v2 = v - dy;
  const double q2 = (d[3] * (u2 * u2) + (d[4] * u2) * v2) + d[5] * (v2 * v2);
  tab[(size_t)s * tabs + k] = (1.0 - q) * dev::exp_neg(q1) + q * dev::exp_neg(q2);
}

// 7. corr: workgroup (x, y, z) = tile x (64 candidate columns, 2 kR candidate rows), phase y,
// sample z; wave w of it the candidate rows cy0 = (2 trow + w) kR ...  Candidate row cy meets
// pixel row iy at table row d = iy - cy; the workgroup walks d over the union of its waves'
// ranges, a wave skips the rows outside its own (its pixel rows then stay inside the zero
// padding).  seg[dd][k] is table column k - 63 - cx0 (0 outside the table: idle lanes'),
// so lane l reads seg[dd][63 - l + ix] for pixel column ix.  nq[sample][2][G].
template <int R>
__global__ __launch_bounds__(kCorrThreads) __attribute__((amdgpu_waves_per_eu(4, 8)))
void detect_corr_kernel(const unsigned long long *__restrict__ words, int mode,
                        const double *__restrict__ tab, const double2 *__restrict__ zw, int n,
                        int os, int gs, size_t tabs, size_t zws, double *__restrict__ nq) {
  __shared__ double seg[kD][kSegW];
  const int s = blockIdx.z;
  if (s >= work_count(words, mode)) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tx = (n + 63) >> 6;
  const int trow = blockIdx.x / tx, tcol = blockIdx.x - trow * tx;
  const int ph = blockIdx.y, py = ph / os, px = ph - py * os;
  const int T = 2 * n - 1, W = n + 63;
  const double *P = tab + (size_t)s * tabs + (size_t)ph * T * T;
  const double2 *Z = zw + (size_t)s * zws + (size_t)kPad * n;      // pixel row 0
  const int cx0 = tcol * 64, cyw = trow * kCorrWaves * R, cy0 = cyw + wave * R;
  const int dlo = max(-(n - 1), -(cyw + kCorrWaves * R - 1)), dhi = n - 1 - cyw;
  const bool live = cy0 < n;
  const int mylo = -(cy0 + R - 1), myhi = n - 1 - cy0;
  double aN[R], aQ[R];
#pragma unroll
  for (int r = 0; r < R; ++r) aN[r] = aQ[r] = 0.0;
  for (int d0 = dlo; d0 <= dhi; d0 += kD) {
    __syncthreads();
    for (int k = threadIdx.x; k < kD * W; k += kCorrThreads) {
      const int dd = k / W, col = k - dd * W;
      const int d = d0 + dd, tc = col - 63 - cx0 + n - 1;
      seg[dd][col] = d <= dhi && tc >= 0 && tc < T ? P[(size_t)(d + n - 1) * T + tc] : 0.0;
    }
    __syncthreads();
    if (!live) continue;
    for (int dd = 0; dd < kD; ++dd) {
      const int d = d0 + dd;
      if (d < mylo || d > myhi) continue;
      const double2 *zr = Z + (ptrdiff_t)(d + cy0) * n;
      const double *sp = &seg[dd][63 - lane];
#pragma unroll 4
      for (int ix = 0; ix < n; ++ix) {
        const double pv = sp[ix];
        const double p2 = pv * pv;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double2 t = zr[(ptrdiff_t)r * n + ix];
          aN[r] = fma(t.x, pv, aN[r]);
          aQ[r] = fma(t.y, p2, aQ[r]);
        }
      }
    }
  }
  const size_t G = (size_t)gs * gs;
  double *o = nq + (size_t)s * 2 * G;
  const int cx = cx0 + lane, jx = os * cx + px;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int cy = cy0 + r, jy = os * cy + py;
    if (cx < n && cy < n && jx < gs && jy < gs) {
      o[(size_t)jy * gs + jx] = aN[r];
      o[G + (size_t)jy * gs + jx] = aQ[r];
    }
  }
}

// 3. the planes of the one vector in slot 0: A, sigma_A, snr
__global__ __launch_bounds__(kThreads) void detect_planes_kernel(
    const unsigned long long *__restrict__ words, int mode, const double *__restrict__ nq,
    size_t G, double *__restrict__ out) {
  if (!work_count(words, mode)) return;
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= G) return;
  double A, var, snr;
  amplitude(nq[g], nq[G + g], &A, &var, &snr);
  out[g] = A;
  out[G + g] = nq[G + g] > 0.0 ? 1.0 / sqrt(nq[G + g]) : nan("");
  out[2 * G + g] = snr;
}

// 8. stats: workgroup (x, y) = candidates 256 x .., block y of the piece; part[block][5][G]
__global__ __launch_bounds__(kThreads) void detect_stats_kernel(
    const unsigned long long *__restrict__ words, const double *__restrict__ nq,
    const double *__restrict__ piv, size_t G, double *__restrict__ part) {
  const long long cnt = (long long)words[kWPiece];
  const long long b = blockIdx.y;
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (b * kB >= cnt || g >= G) return;
  const int ns = (int)(cnt - b * kB < kB ? cnt - b * kB : kB);
  const double Ap = piv[g], Sp = piv[2 * G + g];
  const double *p = nq + (size_t)b * kB * 2 * G + g;
  double a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0;
  for (int s = 0; s < ns; ++s) {
    double A, var, snr;
    amplitude(p[(size_t)s * 2 * G], p[(size_t)s * 2 * G + G], &A, &var, &snr);
    const double da = A - Ap, ds = snr - Sp;
    a1 += da;
    a2 = fma(da, da, a2);
    a3 += var;
    a4 += ds;
    a5 = fma(ds, ds, a5);
  }
  double *o = part + (size_t)b * kSums * G + g;
  o[0] = a1;
  o[G] = a2;
  o[2 * G] = a3;
  o[3 * G] = a4;
  o[4 * G] = a5;
}

// 9. reduce: the piece's partials into the running sums, in block order
__global__ __launch_bounds__(kThreads) void detect_reduce_kernel(
    const unsigned long long *__restrict__ words, const double *__restrict__ part, size_t len,
    double *__restrict__ sum) {
  const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= len) return;
  const int nb = (int)((words[kWPiece] + kB - 1) / kB);
  double a = sum[t];
  for (int b = 0; b < nb; ++b) a += part[(size_t)b * len + t];
  sum[t] = a;
}

unsigned blocks_of(size_t len) { return (unsigned)((len + kThreads - 1) / kThreads); }

// steps 6 - 7 on `count` sample slots (`row`: the one vector of the modes but kPiece)
template <int NSRC>
void launch_corr(olpe_detect *d, hipStream_t st, int mode, const RowMap &m, long long s0,
                 int count, const double *row) {
  const int tiles = ((d->n + 63) / 64) * ((d->n + kCorrWaves * kR - 1) / (kCorrWaves * kR));
  hipLaunchKernelGGL((detect_prep_kernel<NSRC>), dim3(blocks_of(d->npix + d->tabs), (unsigned)count),
                     dim3(kThreads), 0, st, d->d_words, mode, m, s0, d->d_idx, row, d->d_desc,
                     d->d_DE, d->n, d->os, d->tabs, d->zws, d->d_tab, d->d_zw);
  hipLaunchKernelGGL((detect_corr_kernel<kR>),
                     dim3((unsigned)tiles, (unsigned)(d->os * d->os), (unsigned)count),
                     dim3(kCorrThreads), 0, st, d->d_words, mode, d->d_tab, d->d_zw, d->n, d->os,
                     d->gs, d->tabs, d->zws, d->d_nq);
}

// the planes [3][G] of the vector at `row` (device) into `out`, under `mode`
template <int NSRC>
void launch_one(olpe_detect *d, hipStream_t st, int mode, const double *row, double *out) {
  hipLaunchKernelGGL((detect_rowdesc_kernel<NSRC>), dim3(1), dim3(64), 0, st, d->d_words, mode,
                     row, d->bkgd_mode, d->d_desc);
  launch_corr<NSRC>(d, st, mode, RowMap{row, 1, 0, 0}, 0, 1, row);
  hipLaunchKernelGGL(detect_planes_kernel, dim3(blocks_of(d->G)), dim3(kThreads), 0, st,
                     d->d_words, mode, d->d_nq, d->G, out);
}

template <int NSRC>
int launch_piece_t(olpe_detect *d, hipStream_t st, const RowMap &m, long long s0, int ns) {
  using L = dev::Layout<NSRC>;
  const int nblk = (ns + kB - 1) / kB;
  BlkInfo *info = (BlkInfo *)d->d_info;
  hipLaunchKernelGGL((resid_scan_kernel<L::NP>), dim3(nblk), dim3(kThreads), 0, st, m, s0, ns, info);
  hipLaunchKernelGGL((resid_book_kernel<L::PS>), dim3(1), dim3(kMaxPieceBlocks), 0, st, m, s0, nblk, info,
                     d->d_boff, d->d_words, d->d_pivot, d->d_best);
  launch_one<NSRC>(d, st, kPivotNew, d->d_pivot, d->d_piv);
  hipLaunchKernelGGL((resid_desc_kernel<NSRC>), dim3(nblk), dim3(kThreads), 0, st, m, s0, ns,
                     d->d_boff, d->bkgd_mode, d->d_desc);
  hipLaunchKernelGGL((detect_index_kernel<L::NP>), dim3(nblk), dim3(kThreads), 0, st, m, s0, ns,
                     d->d_boff, d->d_idx);
  launch_corr<NSRC>(d, st, kPiece, m, s0, ns, nullptr);
  hipLaunchKernelGGL(detect_stats_kernel, dim3(blocks_of(d->G), (unsigned)nblk), dim3(kThreads), 0,
                     st, d->d_words, d->d_nq, d->d_piv, d->G, d->d_part);
  hipLaunchKernelGGL(detect_reduce_kernel, dim3(blocks_of(kSums * d->G)), dim3(kThreads), 0, st,
                     d->d_words, d->d_part, kSums * d->G, d->d_sum);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

// `count` samples of the map on `st`, a piece at a time (a piece is a whole number of
// blocks, so the order of a candidate's additions does not depend on the piece size)
int launch_fold(olpe_detect *d, hipStream_t st, const RowMap &m, long long count) {
  const long long piece = (long long)d->piece_blocks * kB;
  for (long long s0 = 0; s0 < count; s0 += piece) {
    const int ns = (int)std::min(piece, count - s0);
    const int rc = d->nsrc == 2 ? launch_piece_t<2>(d, st, m, s0, ns)
                                : launch_piece_t<3>(d, st, m, s0, ns);
    if (rc) return rc;
  }
  return OLPE_OK;
}

// the planes of the vector at `row` (device) into `out`, on the object's stream (waited for)
int eval_one(olpe_detect *d, const double *row, double *out) {
  if (d->nsrc == 2) launch_one<2>(d, d->stream, kOne, row, out);
  else launch_one<3>(d, d->stream, kOne, row, out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(d->stream));
  return OLPE_OK;
}

// the pivot vector at d_pivot -> its planes
int set_pivot(olpe_detect *d, const double *pivot) {
  HIPCHK(hipMemcpyAsync(d->d_pivot, pivot, (size_t)d->ps * 8, hipMemcpyHostToDevice, d->stream));
  int rc;
  if ((rc = eval_one(d, d->d_pivot, d->d_piv))) return rc;
  unsigned long long one = 1;
  HIPCHK(hipMemcpy(d->d_words + kWHavePivot, &one, 8, hipMemcpyHostToDevice));
  return OLPE_OK;
}

int read_words(olpe_detect *d, unsigned long long *w) {
  HIPCHK(hipMemcpy(w, d->d_words, kWords * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

double nan_median(std::vector<double> &v) {
  v.erase(std::remove_if(v.begin(), v.end(), [](double x) { return x != x; }), v.end());
  if (v.empty()) return nan("");
  const size_t h = v.size() / 2;
  std::nth_element(v.begin(), v.begin() + h, v.end());
  const double hi = v[h];
  if (v.size() & 1) return hi;
  const double lo = *std::max_element(v.begin(), v.begin() + h);
  return 0.5 * (lo + hi);
}

}  // namespace

extern "C" {

int olpe_detect_create(olpe_ctx *c, const double *pivot, int oversample, olpe_detect **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (!c) return set_err(OLPE_EINVAL, "NULL context");
  if (oversample != 1 && oversample != 2 && oversample != 4)
    return set_err(OLPE_EINVAL, "oversample %d: 1, 2 or 4", oversample);
  if (c->n > kMaxSide)
    return set_err(OLPE_EINVAL, "a %dx%d frame: the detection map takes sides up to %d", c->n,
                   c->n, kMaxSide);
  if (pivot && !finite_params(pivot, c->np))
    return set_err(OLPE_EINVAL, "the pivot vector has a non-finite parameter");
  HIPCHK(hipSetDevice(c->device));
  olpe_detect *d = new olpe_detect;
  d->n = c->n;
  d->nsrc = c->nsrc;
  d->bkgd_mode = c->bkgd_mode;
  d->ps = c->ps;
  d->os = oversample;
  d->gs = oversample * (c->n - 1) + 1;
  d->npix = (size_t)c->n * c->n;
  d->G = (size_t)d->gs * d->gs;
  const size_t T = 2 * (size_t)c->n - 1;
  d->tabs = (size_t)oversample * oversample * T * T;
  d->zws = (size_t)(c->n + 2 * kPad) * c->n;
  const size_t per_sample = d->tabs * 8 + d->zws * 16 + 2 * d->G * 8;
  d->piece_blocks = (int)std::min<size_t>(4, std::max<size_t>(1, kWorkBudget / (per_sample * kB)));
  const size_t ks = 12 * (size_t)c->nsrc + 1, pb = (size_t)d->piece_blocks, cap = pb * kB;
  std::vector<double2> de(d->npix);
  int rc = fold_open(d, c->device);
  if (!rc) rc = alloc((void **)&d->d_DE, d->npix * sizeof(double2), "the cutout");
  if (!rc) rc = alloc((void **)&d->d_sum, kSums * d->G * 8, "the shifted sums");
  if (!rc) rc = alloc((void **)&d->d_piv, 3 * d->G * 8, "the pivot planes");
  if (!rc) rc = alloc((void **)&d->d_out, 3 * d->G * 8, "the planes of one vector");
  if (!rc) rc = alloc((void **)&d->d_pivot, (size_t)d->ps * 8, "the pivot vector");
  if (!rc) rc = alloc((void **)&d->d_best, (size_t)d->ps * 8, "the best row");
  if (!rc) rc = alloc((void **)&d->d_vec, (size_t)d->ps * 8, "the point vector");
  if (!rc) rc = alloc((void **)&d->d_words, kWords * 8, "the counters");
  if (!rc) rc = alloc(&d->d_info, pb * sizeof(BlkInfo), "the block table");
  if (!rc) rc = alloc((void **)&d->d_boff, pb * sizeof(int), "the block offsets");
  if (!rc) rc = alloc((void **)&d->d_idx, cap * sizeof(int), "the sample index");
  if (!rc) rc = alloc((void **)&d->d_desc, cap * ks * 8, "the sample descriptors");
  if (!rc) rc = alloc((void **)&d->d_tab, cap * d->tabs * 8, "the PSF tables");
  if (!rc) rc = alloc((void **)&d->d_zw, cap * d->zws * sizeof(double2), "the weighted residuals");
  if (!rc) rc = alloc((void **)&d->d_nq, cap * 2 * d->G * 8, "the correlations");
  if (!rc) rc = alloc((void **)&d->d_part, pb * kSums * d->G * 8, "the partial sums");
  // the cutout behind whatever the context's stream still has in flight; the padding rows
  // of the {z, w} planes are zero from here on (prep writes the pixel rows only)
  if (!rc && (hipStreamSynchronize(olpe_main(c)) != hipSuccess ||
              hipMemcpy(d->d_DE, c->d_DE, d->npix * sizeof(double2), hipMemcpyDeviceToDevice) != hipSuccess ||
              hipMemcpy(de.data(), d->d_DE, d->npix * sizeof(double2), hipMemcpyDeviceToHost) != hipSuccess ||
              hipMemset(d->d_zw, 0, cap * d->zws * sizeof(double2)) != hipSuccess ||
              hipMemset(d->d_sum, 0, kSums * d->G * 8) != hipSuccess ||
              hipMemset(d->d_piv, 0, 3 * d->G * 8) != hipSuccess ||
              hipMemset(d->d_pivot, 0, (size_t)d->ps * 8) != hipSuccess ||
              hipMemset(d->d_best, 0, (size_t)d->ps * 8) != hipSuccess ||
              hipMemset(d->d_words, 0, kWords * 8) != hipSuccess ||
              hipDeviceSynchronize() != hipSuccess))
    rc = set_err(OLPE_EHIP, "cutout copy failed");
  for (const double2 &p : de) d->pixels += p.y != 0.0;
  if (!rc && pivot) {
    std::vector<double> pv(pivot, pivot + c->np);
    pv.push_back(0.0);                          // the chi^2 column plays no part
    rc = set_pivot(d, pv.data());
    d->explicit_pivot = true;
  }
  if (rc) {
    olpe_detect_destroy(d);
    return rc;
  }
  *out = d;
  return OLPE_OK;
}

void olpe_detect_destroy(olpe_detect *d) {
  if (!d) return;
  fold_close(d, {d->d_DE, d->d_sum, d->d_piv, d->d_out, d->d_pivot, d->d_best, d->d_vec,
                 d->d_words, d->d_info, d->d_boff, d->d_idx, d->d_desc, d->d_tab, d->d_zw,
                 d->d_nq, d->d_part, d->d_stage});
  delete d;
}

int olpe_detect_fold_ctx(olpe_detect *d, olpe_ctx *c, int row_step, int walker_step) {
  if (!d || !c) return set_err(OLPE_EINVAL, "NULL argument");
  if (row_step <= 0 || walker_step <= 0)
    return set_err(OLPE_EINVAL, "row_step %d, walker_step %d: both must be > 0", row_step,
                   walker_step);
  if (c->device != d->device || c->n != d->n || c->nsrc != d->nsrc || c->bkgd_mode != d->bkgd_mode)
    return set_err(OLPE_EINVAL, "context of device %d, side %d, %d sources, bkgd_mode %d; this "
                   "object of device %d, side %d, %d sources, bkgd_mode %d", c->device, c->n,
                   c->nsrc, c->bkgd_mode, d->device, d->n, d->nsrc, d->bkgd_mode);
  int rc;
  if ((rc = fold_check(d, c))) return rc;
  HIPCHK(hipSetDevice(d->device));
  // rows 0, row_step, ... of walkers 0, walker_step, ... of the chain [W][nrec][PS],
  // walker-major: indexing only
  const long long nr = (c->chain_rows + row_step - 1) / row_step;
  const long long nw = ((long long)c->W + walker_step - 1) / walker_step;
  const RowMap m{c->d_chain, nr, (long long)walker_step * c->chain_rows * c->ps,
                 (long long)row_step * c->ps};
  return fold_run(d, c, nr > 0 && nw > 0,
                  [&](hipStream_t s) { return launch_fold(d, s, m, nr * nw); });
}

int olpe_detect_fold_rows(olpe_detect *d, const double *rows, long long nsamples) {
  if (!d) return set_err(OLPE_EINVAL, "NULL argument");
  if (nsamples < 0 || (nsamples > 0 && !rows))
    return set_err(OLPE_EINVAL, "%lld samples at %p", nsamples, (const void *)rows);
  if (nsamples == 0) return OLPE_OK;
  HIPCHK(hipSetDevice(d->device));
  const long long piece = (long long)d->piece_blocks * kB;
  int rc;
  if (!d->d_stage &&
      (rc = alloc((void **)&d->d_stage, (size_t)piece * d->ps * 8, "the row upload")))
    return rc;
  if ((rc = wait_pending(d))) return rc;
  for (long long s0 = 0; s0 < nsamples; s0 += piece) {
    const long long ns = std::min(piece, nsamples - s0);
    HIPCHK(hipMemcpyAsync(d->d_stage, rows + (size_t)s0 * d->ps, (size_t)ns * d->ps * 8,
                          hipMemcpyHostToDevice, d->stream));
    const RowMap m{d->d_stage, ns, 0, (long long)d->ps};
    if ((rc = launch_fold(d, d->stream, m, ns))) return rc;
    HIPCHK(hipStreamSynchronize(d->stream));   // d_stage is reused
  }
  return OLPE_OK;
}

int olpe_detect_get(olpe_detect *d, long long *n, long long *n_bad, double *pivot, double *sums,
                    double *best) {
  if (!d) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(d->device));
  int rc;
  if ((rc = drain(d))) return rc;
  unsigned long long w[kWords];
  if ((rc = read_words(d, w))) return rc;
  if (n) *n = (long long)w[kWUsed];
  if (n_bad) *n_bad = (long long)w[kWBad];
  if (pivot) {
    if (w[kWHavePivot]) HIPCHK(hipMemcpy(pivot, d->d_pivot, (size_t)d->ps * 8, hipMemcpyDeviceToHost));
    else for (int k = 0; k < d->ps; ++k) pivot[k] = nan("");
  }
  if (sums) HIPCHK(hipMemcpy(sums, d->d_sum, kSums * d->G * 8, hipMemcpyDeviceToHost));
  if (best) {
    if (w[kWHaveBest]) HIPCHK(hipMemcpy(best, d->d_best, (size_t)d->ps * 8, hipMemcpyDeviceToHost));
    else for (int k = 0; k < d->ps; ++k) best[k] = nan("");
  }
  return OLPE_OK;
}

int olpe_detect_add(olpe_detect *d, long long n, long long n_bad, const double *pivot,
                    const double *sums, const double *best) {
  if (!d || !pivot || !sums || !best) return set_err(OLPE_EINVAL, "NULL argument");
  if (n < 0 || n_bad < 0) return set_err(OLPE_EINVAL, "n %lld, n_bad %lld", n, n_bad);
  HIPCHK(hipSetDevice(d->device));
  int rc;
  if ((rc = drain(d))) return rc;
  unsigned long long w[kWords];
  if ((rc = read_words(d, w))) return rc;
  if (n > 0) {
    std::vector<double> cur((size_t)d->ps);
    HIPCHK(hipMemcpy(cur.data(), d->d_pivot, (size_t)d->ps * 8, hipMemcpyDeviceToHost));
    if (w[kWUsed] == 0) {
      // empty: the incoming pivot becomes this object's
      if (!finite_params(pivot, d->ps - 1))
        return set_err(OLPE_EINVAL, "the incoming pivot has a non-finite parameter");
      if (!w[kWHavePivot] || memcmp(cur.data(), pivot, (size_t)(d->ps - 1) * 8)) {
        if ((rc = set_pivot(d, pivot))) return rc;
        d->explicit_pivot = false;
      }
    } else if (memcmp(cur.data(), pivot, (size_t)(d->ps - 1) * 8)) {
      return set_err(OLPE_EINVAL, "the pivots differ: sums about different planes do not add");
    }
    const size_t len = kSums * d->G;
    std::vector<double> sum(len);
    HIPCHK(hipMemcpy(sum.data(), d->d_sum, len * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < len; ++i) sum[i] += sums[i];
    HIPCHK(hipMemcpy(d->d_sum, sum.data(), len * 8, hipMemcpyHostToDevice));
    // this object's folds come first: the incoming best wins only if strictly smaller
    const double chi = best[d->ps - 1];
    if (chi == chi) {
      double mine = 0.0;
      if (w[kWHaveBest])
        HIPCHK(hipMemcpy(&mine, d->d_best + d->ps - 1, 8, hipMemcpyDeviceToHost));
      if (!w[kWHaveBest] || chi < mine) {
        HIPCHK(hipMemcpy(d->d_best, best, (size_t)d->ps * 8, hipMemcpyHostToDevice));
        w[kWHaveBest] = 1;
      }
    }
  }
  w[kWUsed] += (unsigned long long)n;
  w[kWBad] += (unsigned long long)n_bad;
  HIPCHK(hipMemcpy(d->d_words + kWUsed, &w[kWUsed], 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d->d_words + kWBad, &w[kWBad], 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d->d_words + kWHaveBest, &w[kWHaveBest], 8, hipMemcpyHostToDevice));
  return OLPE_OK;
}

int olpe_detect_reset(olpe_detect *d) {
  if (!d) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(d->device));
  int rc;
  if ((rc = drain(d))) return rc;
  unsigned long long w[kWords] = {};
  w[kWHavePivot] = d->explicit_pivot;          // a pivot given at create stays
  HIPCHK(hipMemset(d->d_sum, 0, kSums * d->G * 8));
  HIPCHK(hipMemcpy(d->d_words, w, kWords * 8, hipMemcpyHostToDevice));
  fold_forget(d);
  return OLPE_OK;
}

int olpe_detect_point(olpe_detect *d, const double *vec, double *planes) {
  if (!d || !vec || !planes) return set_err(OLPE_EINVAL, "NULL argument");
  if (!finite_params(vec, d->ps - 1))
    return set_err(OLPE_EINVAL, "the vector has a non-finite parameter");
  HIPCHK(hipSetDevice(d->device));
  int rc;
  if ((rc = drain(d))) return rc;
  HIPCHK(hipMemcpy(d->d_vec, vec, (size_t)(d->ps - 1) * 8, hipMemcpyHostToDevice));
  if ((rc = eval_one(d, d->d_vec, d->d_out))) return rc;
  HIPCHK(hipMemcpy(planes, d->d_out, 3 * d->G * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

int olpe_detect_finalize(olpe_detect *d, double *planes, double *scalars) {
  if (!d || !planes || !scalars) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(d->device));
  int rc;
  if ((rc = drain(d))) return rc;
  unsigned long long w[kWords];
  if ((rc = read_words(d, w))) return rc;
  if (w[kWUsed] == 0)
    return set_err(OLPE_ESTATE, "no usable sample folded (%llu unusable)", w[kWBad]);
  if (!w[kWHaveBest])
    return set_err(OLPE_ESTATE, "the chi^2 column of all %llu usable samples is NaN: no best "
                   "sample", w[kWUsed]);
  const size_t G = d->G;
  if ((rc = eval_one(d, d->d_best, d->d_out))) return rc;
  std::vector<double> sum(kSums * G), piv(3 * G);
  HIPCHK(hipMemcpy(sum.data(), d->d_sum, kSums * G * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(piv.data(), d->d_piv, 3 * G * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(planes + 7 * G, d->d_out, 3 * G * 8, hipMemcpyDeviceToHost));
  // detect.py's planes_from_state restates this arithmetic
  const double nu = (double)w[kWUsed];
  long long blind = 0, at = -1;
  double hi = nan(""), lo = nan("");
  std::vector<double> tot(G);
  for (size_t g = 0; g < G; ++g) {
    const double m1 = sum[g] / nu;
    const double va = (sum[G + g] - sum[g] * m1) / nu;
    const double vac = va < 0.0 ? 0.0 : va;
    const double ms = sum[2 * G + g] / nu;
    const double m4 = sum[3 * G + g] / nu;
    const double vs = (sum[4 * G + g] - sum[3 * G + g] * m4) / nu;
    const double mean = piv[g] + m1;
    tot[g] = sqrt(ms + vac);
    planes[g] = mean;
    planes[G + g] = sqrt(vac);
    planes[2 * G + g] = sqrt(ms);
    planes[3 * G + g] = tot[g];
    planes[4 * G + g] = piv[2 * G + g] + m4;
    planes[5 * G + g] = sqrt(vs < 0.0 ? 0.0 : vs);
    const double marg = mean / tot[g];
    planes[6 * G + g] = marg;
    blind += ms != ms;
    if (marg == marg) {
      if (!(marg <= hi)) {                      // the lowest candidate on a tie
        hi = marg;
        at = (long long)g;
      }
      if (!(marg >= lo)) lo = marg;
    }
  }
  scalars[0] = nu;
  scalars[1] = (double)w[kWBad];
  scalars[2] = (double)d->pixels;
  scalars[3] = (double)blind;
  scalars[4] = hi;
  scalars[5] = (double)at;
  scalars[6] = lo;
  scalars[7] = nan_median(tot);
  return OLPE_OK;
}

}  // extern "C"

// olpe_internal.h: the hand-over to olpe_detnull.hip
int olpe_detect_view_at(olpe_detect *d, const double *vec, olpe_detect_view *v) {
  *v = olpe_detect_view{d->device, d->n, d->os, d->gs, d->ps, d->tabs, nullptr, nullptr, nullptr,
                        nullptr};
  if (!vec) return OLPE_OK;
  HIPCHK(hipSetDevice(d->device));
  int rc;
  if ((rc = drain(d))) return rc;
  HIPCHK(hipMemcpy(d->d_vec, vec, (size_t)(d->ps - 1) * 8, hipMemcpyHostToDevice));
  if ((rc = eval_one(d, d->d_vec, d->d_out))) return rc;
  v->tab = d->d_tab;
  v->DE = d->d_DE;
  v->Q = d->d_nq + d->G;
  v->sigma = d->d_out + d->G;
  return OLPE_OK;
}
