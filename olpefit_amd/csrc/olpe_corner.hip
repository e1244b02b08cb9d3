// olpe_corner.hip -- the data behind the reference's corner plot (apf_step3.py:603-643;
// 3body/apf_step3_3body.py likewise): a fine 1-D histogram per column and a coarse 2-D
// histogram per pair of columns of the recorded rows, counted on the device.
//
// An olpe_corner belongs to a device, not to a sampler context.  It holds both edge sets
// and one array of 64-bit counters, h1 [ncols][nb1] followed by h2 [npairs][nb2][nb2].
// Counts are integers and additive: they stream launch by launch, need no sample store
// and do not depend on how the rows were split, on the grid or on the tiling.
//   * A workgroup owns a tile -- a contiguous range of the counters that fits LDS (some
//     columns' 1-D histograms, or some pairs' 2-D ones) -- and a chunk of the samples.
//     It counts into 32-bit LDS counters (a chunk is at most kMaxChunk samples, so no
//     counter can wrap) and adds the non-zero ones to the global counters with 64-bit
//     integer atomics.  The rows are re-read per tile (from L2).
//   * The 2-D kernel takes 512 samples at a time: their [512][ncols] values are read in
//     memory order and each one's coarse bin is found (bytes in LDS, 0xFF = no bin), then
//     the increments run in one of two lane layouts: a lane per sample (every lane walks
//     the tile's pairs), or a lane per pair (a wave's lanes cover distinct pairs of a few
//     samples, so the addresses of one instruction differ by construction).  DESIGN.md
//     §7c has the A/B.
// The bin rule is NumPy's (np.histogram / np.histogram2d with explicit edges): bin k iff
// e[k] <= x < e[k+1], the last edge in the last bin, anything else (NaN, +-inf included)
// in no bin.  Only comparisons with the uploaded edges decide; the computed first guess
// is a shortcut.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/olpe.h"
#include "olpe_fold.h"
#include "olpe_internal.h"

using namespace olpe;

struct olpe_corner : FoldBase {
  int ncols = 0, nb1 = 0, nb2 = 0, npairs = 0;
  int cpt = 0, ntiles1 = 0;     // columns per 1-D tile, tiles
  int ppt = 0, ntiles2 = 0;     // pairs per 2-D tile, tiles
  size_t lds1 = 0, lds2 = 0;    // dynamic LDS bytes of the two kernels
  int form = 1;                 // 2-D increments: 0 = a lane per sample, 1 = a lane per pair
  unsigned long long n = 0;     // samples folded
  size_t ncount = 0;            // ncols * nb1 + npairs * nb2 * nb2
  double *d_e1 = nullptr, *d_e2 = nullptr;   // [ncols][nb1 + 1], [ncols][nb2 + 1]
  double2 *d_g1 = nullptr, *d_g2 = nullptr;  // per column {first edge, bins per unit}
  unsigned short *d_tab = nullptr;           // [npairs] (i << 8) | j
  unsigned long long *d_cnt = nullptr;       // [ncount]
  double *d_stage = nullptr;                 // upload staging of fold_rows
};

namespace {

constexpr int kThreads = 512;
constexpr int kMaxCols = 24, kMaxNb1 = 4096, kMaxNb2 = 64;
constexpr size_t kLdsBudget = 64 * 1024;           // per workgroup, both kernels
constexpr long long kMaxChunk = 1ll << 24;         // samples per workgroup: < 2^32 per counter
constexpr long long kStageSamples = 1ll << 18;     // fold_rows uploads this many samples a piece
constexpr unsigned kNoBin = 0xFFu;
// LDS strides that spread a wave over the banks: lanes on different pairs (columns) and
// the same bins (sample) would otherwise share a bank -- 400 counters are 16 banks apart
// twice over, 512 bytes none at all
constexpr int kBinStride = kThreads + 4;           // bytes per column of the batch's bins
__host__ __device__ constexpr int pair_stride(int nb2) { return (nb2 * nb2) | 1; }

// The bin of x among the strictly increasing edges e[0 .. nb]: -1 if it has none.
// g = {e[0], nb / (e[nb] - e[0])} gives a first guess that is right (or one off) for
// evenly spaced edges; the comparisons with e[k], e[k+1] decide, and a bisection of at
// most 13 steps (nb <= 4096) finds the bin for any other edges.
__device__ __forceinline__ int find_bin(const double *__restrict__ e, int nb, double x, double2 g) {
  const double t = (x - g.x) * g.y;
  const int k = t >= 0.0 ? (t >= (double)(nb - 1) ? nb - 1 : (int)t) : 0;   // NaN -> 0
  const double ek = e[k], ek1 = e[k + 1];
  if (ek <= x && x < ek1) return k;                // the guess was right: two loads
  if (!(x >= e[0] && x <= e[nb])) return -1;       // below, above, NaN, +-inf
  if (x >= e[nb - 1]) return nb - 1;               // the last bin is closed on the right
  if (x >= ek1) {
    if (k + 2 <= nb && x < e[k + 2]) return k + 1;
  } else if (k > 0 && e[k - 1] <= x) {             // x < e[k] here
    return k - 1;
  }
  int a = 0, b = nb - 1;                           // e[a] <= x < e[b]
  for (int it = 0; it < 13 && b - a > 1; ++it) {
    const int m = (a + b) >> 1;
    if (x >= e[m]) a = m; else b = m;
  }
  return a;
}

// h1: tile t = columns [t * cpt, ...).  A thread per (sample, column) item of the chunk's
// [samples][nc] block, adjacent lanes on adjacent columns, so a wave reads the tile's
// share of a dozen consecutive rows, not one value of 64 rows.  2,048 fine bins spread a
// posterior over hundreds of addresses: same-address LDS atomics are rare here.
__global__ __launch_bounds__(kThreads) void corner_fold1_kernel(
    const double *__restrict__ rows, long long n, int C, int nb1,
    const double *__restrict__ edges, const double2 *__restrict__ guess, int cpt,
    long long chunk, unsigned long long *__restrict__ h1) {
  extern __shared__ unsigned cnt1[];
  const int c0 = blockIdx.y * cpt;
  const int nc = min(cpt, C - c0);
  const int ncnt = nc * nb1;
  for (int i = threadIdx.x; i < ncnt; i += kThreads) cnt1[i] = 0;
  __syncthreads();
  const long long s0 = (long long)blockIdx.x * chunk;
  const long long s1 = s0 + chunk < n ? s0 + chunk : n;
  const int step_c = kThreads % nc, step_s = kThreads / nc;
  int c = threadIdx.x % nc;
  long long s = s0 + threadIdx.x / nc;
  while (s < s1) {
    const int col = c0 + c;
    const int k = find_bin(edges + (size_t)col * (nb1 + 1), nb1, rows[(size_t)s * C + col],
                           guess[col]);
    if (k >= 0 && k < nb1) atomicAdd(&cnt1[c * nb1 + k], 1u);
    c += step_c;
    s += step_s;
    if (c >= nc) {
      c -= nc;
      ++s;
    }
  }
  __syncthreads();
  unsigned long long *out = h1 + (size_t)c0 * nb1;
  for (int i = threadIdx.x; i < ncnt; i += kThreads)
    if (cnt1[i]) atomicAdd(&out[i], (unsigned long long)cnt1[i]);
}

// h2: tile t = pairs [t * ppt, ...).  LDS: the coarse edges and guesses, the tile's
// counters, its pair table and the 512 samples' bins [column][sample].
template <bool kLanePerPair>
__global__ __launch_bounds__(kThreads) void corner_fold2_kernel(
    const double *__restrict__ rows, long long n, int C, int nb2,
    const double *__restrict__ edges, const double2 *__restrict__ guess,
    const unsigned short *__restrict__ tab, int npairs, int ppt, long long chunk,
    unsigned long long *__restrict__ h2) {
  extern __shared__ double smem2[];
  double *e = smem2;                                             // [C][nb2 + 1]
  double *g = e + C * (nb2 + 1);                                 // [C][2]
  unsigned *cnt = (unsigned *)(g + 2 * C);                       // [npt][nb2][nb2]
  const int p0 = blockIdx.y * ppt;
  const int npt = min(ppt, npairs - p0);
  const int nn = nb2 * nb2, nns = pair_stride(nb2);
  const int ncnt = npt * nn;
  unsigned short *ptab = (unsigned short *)(cnt + ppt * nns);    // [npt]
  unsigned char *bins = (unsigned char *)(ptab + ((ppt + 3) & ~3));  // [C][kBinStride]
  for (int i = threadIdx.x; i < C * (nb2 + 1); i += kThreads) e[i] = edges[i];
  for (int i = threadIdx.x; i < C; i += kThreads) {
    g[2 * i] = guess[i].x;
    g[2 * i + 1] = guess[i].y;
  }
  for (int i = threadIdx.x; i < npt * nns; i += kThreads) cnt[i] = 0;
  for (int i = threadIdx.x; i < npt; i += kThreads) ptab[i] = tab[p0 + i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char *wb = bins + wave * 64;                          // this wave's 64 samples
  const long long s0 = (long long)blockIdx.x * chunk;
  const long long s1 = s0 + chunk < n ? s0 + chunk : n;
  // the lane-per-pair walk over the wave's 64 x npt (sample, pair) items, 64 at a time
  const int step_p = 64 % npt, step_s = 64 / npt;
  // the bin phase's walk over a batch's [512][C] values, 512 consecutive ones at a time
  const int bstep_c = kThreads % C, bstep_s = kThreads / C;
  const int bc0 = threadIdx.x % C, bs0 = threadIdx.x / C;
  for (long long base = s0; base < s1; base += kThreads) {
    int c = bc0, sb = bs0;
    for (int it = 0; it < C; ++it) {
      const bool act = base + sb < s1;
      const int k = act ? find_bin(e + c * (nb2 + 1), nb2, rows[(size_t)(base + sb) * C + c],
                                   make_double2(g[2 * c], g[2 * c + 1]))
                        : -1;
      bins[c * kBinStride + sb] = (unsigned char)(k >= 0 && k < nb2 ? (unsigned)k : kNoBin);
      c += bstep_c;
      sb += bstep_s;
      if (c >= C) {
        c -= C;
        ++sb;
      }
    }
    __syncthreads();
    // four items a pass, their loads ahead of their atomics (LDS latency overlaps)
    if (kLanePerPair) {
      int p = lane % npt, sl = lane / npt;
      while (sl < 64) {
        int pp[4];
        unsigned bi[4], bj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          pp[u] = p;
          const bool ok = sl < 64;
          const int ss = ok ? sl : 63;
          const unsigned ij = ptab[p];
          const unsigned vi = wb[(ij >> 8) * kBinStride + ss], vj = wb[(ij & 255u) * kBinStride + ss];
          bi[u] = ok ? vi : kNoBin;
          bj[u] = ok ? vj : kNoBin;
          p += step_p;
          sl += step_s;
          if (p >= npt) {
            p -= npt;
            ++sl;
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (bi[u] < (unsigned)nb2 && bj[u] < (unsigned)nb2)
            atomicAdd(&cnt[pp[u] * nns + bi[u] * nb2 + bj[u]], 1u);
      }
    } else {
      for (int p = 0; p < npt; p += 4) {
        unsigned bi[4], bj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool ok = p + u < npt;
          const unsigned ij = ptab[ok ? p + u : p];
          const unsigned vi = wb[(ij >> 8) * kBinStride + lane],
                       vj = wb[(ij & 255u) * kBinStride + lane];
          bi[u] = ok ? vi : kNoBin;
          bj[u] = ok ? vj : kNoBin;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (bi[u] < (unsigned)nb2 && bj[u] < (unsigned)nb2)
            atomicAdd(&cnt[(p + u) * nns + bi[u] * nb2 + bj[u]], 1u);
      }
    }
    __syncthreads();
  }
  unsigned long long *out = h2 + (size_t)p0 * nn;
  for (int i = threadIdx.x; i < ncnt; i += kThreads) {
    const int p = i / nn;
    const unsigned v = cnt[p * nns + (i - p * nn)];
    if (v) atomicAdd(&out[i], (unsigned long long)v);
  }
}

size_t lds2_bytes(int ncols, int nb2, int ppt) {
  return (size_t)ncols * (nb2 + 1) * 8 + (size_t)ncols * 16 + (size_t)ppt * pair_stride(nb2) * 4 + (size_t)((ppt + 3) & ~3) * 2 +
         (size_t)ncols * kBinStride;
}

// `what` names the edge set in the message
int check_edges(const double *e, int ncols, int nb, const char *what) {
  for (int c = 0; c < ncols; ++c) {
    const double *ec = e + (size_t)c * (nb + 1);
    for (int k = 0; k <= nb; ++k) {
      if (!isfinite(ec[k]))
        return set_err(OLPE_EINVAL, "column %d: %s edge %d is not finite", c, what, k);
      if (k && !(ec[k] > ec[k - 1]))
        return set_err(OLPE_EINVAL, "column %d: %s edges %d and %d are not strictly increasing "
                       "(%.17g, %.17g)", c, what, k - 1, k, ec[k - 1], ec[k]);
    }
  }
  return OLPE_OK;
}

std::vector<double2> guesses(const double *e, int ncols, int nb) {
  std::vector<double2> g((size_t)ncols);
  for (int c = 0; c < ncols; ++c) {
    const double lo = e[(size_t)c * (nb + 1)], hi = e[(size_t)c * (nb + 1) + nb];
    const double inv = (double)nb / (hi - lo);     // a span that overflows gives 0: guess 0
    g[c] = make_double2(lo, isfinite(inv) ? inv : 0.0);
  }
  return g;
}

// the two fold kernels over n samples [n][ncols] at d_rows, on `stream`
int launch_fold(olpe_corner *h, hipStream_t stream, const double *d_rows, long long n) {
  // enough workgroups to fill the chip, few enough that a tile's flush stays small
  // beside its counting; never more than kMaxChunk samples per workgroup
  const long long tiles = std::max(h->ntiles1, h->ntiles2);
  long long chunks = std::min((n + 4095) / 4096, std::max(1ll, 2048 / tiles));
  long long chunk = (n + chunks - 1) / chunks;
  chunk = std::min(kMaxChunk, (chunk + kThreads - 1) / kThreads * kThreads);
  chunks = (n + chunk - 1) / chunk;
  if (chunks > 0x7fffffffll) return set_err(OLPE_EINVAL, "%lld samples in one fold", n);
  hipLaunchKernelGGL(corner_fold1_kernel, dim3((unsigned)chunks, (unsigned)h->ntiles1),
                     dim3(kThreads), h->lds1, stream, d_rows, n, h->ncols, h->nb1, h->d_e1,
                     h->d_g1, h->cpt, chunk, h->d_cnt);
  HIPCHK(hipGetLastError());
  unsigned long long *h2 = h->d_cnt + (size_t)h->ncols * h->nb1;
  const dim3 grid((unsigned)chunks, (unsigned)h->ntiles2);
  if (h->form)
    hipLaunchKernelGGL(corner_fold2_kernel<true>, grid, dim3(kThreads), h->lds2, stream, d_rows,
                       n, h->ncols, h->nb2, h->d_e2, h->d_g2, h->d_tab, h->npairs, h->ppt, chunk,
                       h2);
  else
    hipLaunchKernelGGL(corner_fold2_kernel<false>, grid, dim3(kThreads), h->lds2, stream, d_rows,
                       n, h->ncols, h->nb2, h->d_e2, h->d_g2, h->d_tab, h->npairs, h->ppt, chunk,
                       h2);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_corner_create(int device, int ncols, const double *edges1, int nb1,
                       const double *edges2, int nb2, olpe_corner **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (ncols < 2 || ncols > kMaxCols)
    return set_err(OLPE_EINVAL, "ncols %d: 2 to %d columns", ncols, kMaxCols);
  if (nb1 < 2 || nb1 > kMaxNb1)
    return set_err(OLPE_EINVAL, "nb1 %d: 2 to %d bins of the 1-D histograms", nb1, kMaxNb1);
  if (nb2 < 2 || nb2 > kMaxNb2)
    return set_err(OLPE_EINVAL, "nb2 %d: 2 to %d bins per axis of the 2-D histograms", nb2,
                   kMaxNb2);
  if (!edges1 || !edges2) return set_err(OLPE_EINVAL, "NULL edges");
  int rc;
  if ((rc = check_edges(edges1, ncols, nb1, "1-D"))) return rc;
  if ((rc = check_edges(edges2, ncols, nb2, "2-D"))) return rc;
  // the smallest tiles: one column's 1-D histogram, one pair's 2-D one
  const size_t min1 = (size_t)nb1 * 4, min2 = lds2_bytes(ncols, nb2, 1);
  if (min1 > kLdsBudget || min2 > kLdsBudget)
    return set_err(OLPE_EINVAL, "the smallest tile needs %zu bytes of LDS (%d columns, nb1 %d, "
                   "nb2 %d); a workgroup has %zu", std::max(min1, min2), ncols, nb1, nb2,
                   kLdsBudget);
  int form = 1;
  if (const char *f = getenv("OLPE_CORNER_FORM")) {
    if (!strcmp(f, "sample")) form = 0;
    else if (!strcmp(f, "pair")) form = 1;
    else return set_err(OLPE_EINVAL, "OLPE_CORNER_FORM=%s: sample or pair", f);
  }
  if ((rc = open_device(device))) return rc;
  olpe_corner *h = new olpe_corner;
  h->ncols = ncols;
  h->nb1 = nb1;
  h->nb2 = nb2;
  h->npairs = ncols * (ncols - 1) / 2;
  h->form = form;
  // tiles of even size, each within the budget
  const int cmax = (int)std::min<size_t>(ncols, kLdsBudget / min1);
  h->ntiles1 = (ncols + cmax - 1) / cmax;
  h->cpt = (ncols + h->ntiles1 - 1) / h->ntiles1;
  h->ntiles1 = (ncols + h->cpt - 1) / h->cpt;
  h->lds1 = (size_t)h->cpt * nb1 * 4;
  int pmax = 1;
  while (pmax < h->npairs && lds2_bytes(ncols, nb2, pmax + 1) <= kLdsBudget) ++pmax;
  h->ntiles2 = (h->npairs + pmax - 1) / pmax;
  h->ppt = (h->npairs + h->ntiles2 - 1) / h->ntiles2;
  h->ntiles2 = (h->npairs + h->ppt - 1) / h->ppt;
  h->lds2 = lds2_bytes(ncols, nb2, h->ppt);
  h->ncount = (size_t)ncols * nb1 + (size_t)h->npairs * nb2 * nb2;
  std::vector<unsigned short> tab;
  for (int i = 0; i < ncols; ++i)
    for (int j = i + 1; j < ncols; ++j) tab.push_back((unsigned short)((i << 8) | j));
  const std::vector<double2> g1 = guesses(edges1, ncols, nb1), g2 = guesses(edges2, ncols, nb2);
  const size_t b1 = (size_t)ncols * (nb1 + 1) * 8, b2 = (size_t)ncols * (nb2 + 1) * 8;
  rc = fold_open(h, device);
  if (!rc) rc = alloc((void **)&h->d_e1, b1, "the 1-D edges");
  if (!rc) rc = alloc((void **)&h->d_e2, b2, "the 2-D edges");
  if (!rc) rc = alloc((void **)&h->d_g1, (size_t)ncols * sizeof(double2), "the 1-D guesses");
  if (!rc) rc = alloc((void **)&h->d_g2, (size_t)ncols * sizeof(double2), "the 2-D guesses");
  if (!rc) rc = alloc((void **)&h->d_tab, tab.size() * 2, "the pair table");
  if (!rc) rc = alloc((void **)&h->d_cnt, h->ncount * 8, "the corner counters");
  if (!rc) rc = alloc((void **)&h->d_stage, (size_t)kStageSamples * ncols * 8, "the row upload");
  if (!rc &&
      (hipMemcpy(h->d_e1, edges1, b1, hipMemcpyHostToDevice) != hipSuccess ||
       hipMemcpy(h->d_e2, edges2, b2, hipMemcpyHostToDevice) != hipSuccess ||
       hipMemcpy(h->d_g1, g1.data(), (size_t)ncols * sizeof(double2), hipMemcpyHostToDevice) !=
           hipSuccess ||
       hipMemcpy(h->d_g2, g2.data(), (size_t)ncols * sizeof(double2), hipMemcpyHostToDevice) !=
           hipSuccess ||
       hipMemcpy(h->d_tab, tab.data(), tab.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
       hipMemset(h->d_cnt, 0, h->ncount * 8) != hipSuccess))
    rc = set_err(OLPE_EHIP, "edge upload failed");
  if (rc) {
    olpe_corner_destroy(h);
    return rc;
  }
  *out = h;
  return OLPE_OK;
}

void olpe_corner_destroy(olpe_corner *h) {
  if (!h) return;
  fold_close(h, {h->d_e1, h->d_e2, h->d_g1, h->d_g2, h->d_tab, h->d_cnt, h->d_stage});
  delete h;
}

int olpe_corner_fold_ctx(olpe_corner *h, olpe_ctx *c) {
  if (!h || !c) return set_err(OLPE_EINVAL, "NULL argument");
  if (c->device != h->device || c->ps != h->ncols)
    return set_err(OLPE_EINVAL, "context of device %d, PS %d; corner of device %d, %d columns",
                   c->device, c->ps, h->device, h->ncols);
  int rc;
  if ((rc = fold_check(h, c))) return rc;
  const long long n = (long long)c->W * c->chain_rows;
  HIPCHK(hipSetDevice(h->device));
  if ((rc = fold_run(h, c, n > 0, [&](hipStream_t s) {
         return launch_fold(h, s, c->d_chain, n);               // [W][nrec][PS]: n rows
       })))
    return rc;
  h->n += (unsigned long long)n;
  return OLPE_OK;
}

int olpe_corner_fold_rows(olpe_corner *h, const double *rows, long long nsamples) {
  if (!h || nsamples < 0 || (nsamples > 0 && !rows)) return set_err(OLPE_EINVAL, "bad argument");
  if (nsamples == 0) return OLPE_OK;
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = wait_pending(h))) return rc;
  for (long long s0 = 0; s0 < nsamples; s0 += kStageSamples) {
    const long long ns = std::min(kStageSamples, nsamples - s0);
    HIPCHK(hipMemcpyAsync(h->d_stage, rows + (size_t)s0 * h->ncols, (size_t)ns * h->ncols * 8,
                          hipMemcpyHostToDevice, h->stream));
    if ((rc = launch_fold(h, h->stream, h->d_stage, ns))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));   // d_stage is reused
    h->n += (unsigned long long)ns;
  }
  return OLPE_OK;
}

int olpe_corner_get(olpe_corner *h, unsigned long long *n, unsigned long long *h1,
                    unsigned long long *h2) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  const size_t n1 = (size_t)h->ncols * h->nb1;
  if (n) *n = h->n;
  if (h1) HIPCHK(hipMemcpy(h1, h->d_cnt, n1 * 8, hipMemcpyDeviceToHost));
  if (h2) HIPCHK(hipMemcpy(h2, h->d_cnt + n1, (h->ncount - n1) * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

int olpe_corner_add(olpe_corner *h, unsigned long long n, const unsigned long long *h1,
                    const unsigned long long *h2) {
  if (!h || !h1 || !h2) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  // 64-bit sums on the host: the counters are a few MB at the most
  const size_t n1 = (size_t)h->ncols * h->nb1;
  std::vector<unsigned long long> cur(h->ncount);
  HIPCHK(hipMemcpy(cur.data(), h->d_cnt, h->ncount * 8, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n1; ++i) cur[i] += h1[i];
  for (size_t i = n1; i < h->ncount; ++i) cur[i] += h2[i - n1];
  HIPCHK(hipMemcpy(h->d_cnt, cur.data(), h->ncount * 8, hipMemcpyHostToDevice));
  h->n += n;
  return OLPE_OK;
}

int olpe_corner_reset(olpe_corner *h) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  HIPCHK(hipMemset(h->d_cnt, 0, h->ncount * 8));
  h->n = 0;
  fold_forget(h);
  return OLPE_OK;
}

}  // extern "C"
