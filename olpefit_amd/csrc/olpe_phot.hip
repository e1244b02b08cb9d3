// olpe_phot.hip -- photometry posteriors of the recorded chains, on the device: the
// companions' flux ratio and delta magnitude, the primary's integrated flux, the PSF's
// FWHM and core fraction per chain row, and their summary (count, extremes, mean, np.std
// and percentile brackets).  The model they are read from is build_analytical_model's
// (apf_step2.py:78-124; 3body/apf_step2_3body.py:78-125): every source shares ampratio
// q, the widths, the angles and the amplitude offset b, so source k integrates to
// F_k = 2 pi (A_k - b) [(1 - q) sx sy + q sx2 sy2].  The FWHM planes are what
// apf_step3.py:463-469 says it takes (the larger sigma); what those lines compute
// (apf_step3.py:454-470) is a host function of olpefit_amd/photometry.py.
//
// An olpe_phot belongs to a device, not to a sampler context.  It stores Q = 2 (nsrc - 1)
// + 5 planes [cap][W] (rows outer, walkers inner, sample (row r, walker w) at r * W + w,
// as the astrometry samples are), plane order: per companion k = 1 .. nsrc - 1
// flux_ratio_k, dmag_k; then flux_primary, fwhm_major, fwhm_minor, fwhm_wide_major,
// core_fraction.
//
// Per row, in this order of IEEE double operations (no contraction: see the pragma), with
// A_k, q, b, sx, sy, sx2, sy2 the row's columns:
//     d0 = A_0 - b
//     usable = every column read is finite, d0 > 0, sx > 0, sy > 0, sx2 > 0, sy2 > 0
//     d_k = A_k - b;  flux_ratio_k = d_k / d0
//     dmag_k = -2.5 * log10(flux_ratio_k) where d_k > 0, else NaN
//     c1 = ((1 - q) * sx) * sy;  c2 = (q * sx2) * sy2;  tot = c1 + c2
//     flux_primary = ((2 pi) * d0) * tot
//     fwhm_major = (2.355 * max(sx, sy)) * pixscale;  fwhm_minor likewise with min
//     fwhm_wide_major = (2.355 * max(sx2, sy2)) * pixscale
//     core_fraction = c1 / tot
// An unusable row stores NaN in every plane and is counted once.  Every NaN stored is the
// positive quiet NaN, which the select keys past every number.  log10 is the device
// library's: it differs from the host's by a few ulp; everything else is
// exact IEEE arithmetic and equals NumPy's bit for bit.
//
// The fold kernel reads rows in contiguous blocks: a workgroup takes a tile of 64 walkers
// x 8 rows, its lanes run over the tile's records in the order they lie in memory (rows
// inner for a sampler's chain [W][rows][PS], walkers inner for host rows [rows][W][PS])
// and each loads one of a record's NC contiguous columns into LDS; then a lane computes a
// sample from its record's columns in LDS and a wave writes 64 walkers of one row, 512
// contiguous bytes per plane.
//
// Finalize reduces the filled prefix of each plane in a fixed order (blocks of kChunk
// samples, a fixed tree inside each, the blocks' partials by one block): the valid count,
// the sum and the extremes' keys, then the squared deviations about the mean (two
// passes, as np.std); NaN takes part in nothing.  The order statistics come from the
// shared radix select (olpe_select.h).
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/olpe.h"
#include "olpe_internal.h"
#include "olpe_reduce.h"
#include "olpe_select.h"
#include "olpe_store.h"

#pragma clang fp contract(off)

using namespace olpe;

// the store holds Q planes; d_part [Q][4][nblk] (sum; count, min, max as words), d_out [Q][4],
// d_words [1] next key
struct olpe_phot : SampleStore {
  int Q = 7;
  double pixscale = 0;
};

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 16;                       // samples per thread of a reduction block
constexpr long long kChunk = kThreads * kPer;  // samples per reduction block
constexpr int kTW = 64, kTR = 8;               // fold tile: walkers x rows
constexpr int kTile = kTW * kTR;               // records per tile, two per thread
constexpr int kColStride = 9;                  // doubles per record in LDS (odd: no bank conflicts)
constexpr int kMaxQ = 9;
constexpr double kTwoPi = 2.0 * M_PI;

// the columns the planes read: a contiguous span of the row (apf_step2.py:78-97;
// 3body :78-98)
template <int NSRC> struct Cols;
template <> struct Cols<2> { static constexpr int first = 6, n = 8; };   // amps .. sigmay2
template <> struct Cols<3> { static constexpr int first = 8, n = 9; };   // ampa .. sigmay2

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double canon(double v) { return v != v ? qnan() : v; }

// One workgroup per tile of kTR rows x kTW walkers.  src element (row r, walker w, column
// c) at w * sw + r * sr + c; rows_inner: records of one walker follow each other in memory
// (sr is the smaller stride).  Sample (row0 + r, w) goes to position (row0 + r) * W + w of
// each plane (N samples apart).
template <int NSRC>
__global__ __launch_bounds__(kThreads) void phot_fold_kernel(
    const double *__restrict__ src, long long sw, long long sr, int rows_inner, long long W,
    long long nrows, long long row0, long long N, double pixscale, double *__restrict__ store,
    unsigned long long *__restrict__ bad) {
  constexpr int NC = Cols<NSRC>::n, C0 = Cols<NSRC>::first, NCOMP = NSRC - 1;
  __shared__ double col[kTile * kColStride];
  const long long r0 = (long long)blockIdx.x * kTR, w0 = (long long)blockIdx.y * kTW;
  // load: flat index f = record * NC + column, the records in memory order
  for (int f = threadIdx.x; f < kTile * NC; f += kThreads) {
    const int j = f / NC, c = f - j * NC;
    const int rl = rows_inner ? (j & (kTR - 1)) : j / kTW;
    const int wl = rows_inner ? j / kTR : (j & (kTW - 1));
    const long long r = r0 + rl, w = w0 + wl;
    if (r < nrows && w < W)
      col[(rl * kTW + wl) * kColStride + c] = src[w * sw + r * sr + C0 + c];
  }
  __syncthreads();
  unsigned nbad = 0;
  for (int s = threadIdx.x; s < kTile; s += kThreads) {
    const int rl = s / kTW, wl = s & (kTW - 1);
    const long long r = r0 + rl, w = w0 + wl;
    if (r >= nrows || w >= W) continue;
    const double *x = col + s * kColStride;
    double A[NSRC];
    for (int k = 0; k < NSRC; ++k) A[k] = x[k];
    const double q = x[NSRC], b = x[NSRC + 1];
    const double sx = x[NSRC + 2], sy = x[NSRC + 3], sx2 = x[NSRC + 4], sy2 = x[NSRC + 5];
    bool ok = isfinite(q) && isfinite(b) && isfinite(sx) && isfinite(sy) && isfinite(sx2) &&
              isfinite(sy2);
    for (int k = 0; k < NSRC; ++k) ok = ok && isfinite(A[k]);
    const double d0 = A[0] - b;
    ok = ok && d0 > 0.0 && sx > 0.0 && sy > 0.0 && sx2 > 0.0 && sy2 > 0.0;
    double v[2 * NCOMP + 5];
    if (ok) {
      for (int k = 1; k < NSRC; ++k) {
        const double dk = A[k] - b;
        const double ratio = dk / d0;
        v[2 * (k - 1)] = ratio;
        v[2 * (k - 1) + 1] = dk > 0.0 ? -2.5 * log10(ratio) : qnan();
      }
      const double c1 = ((1.0 - q) * sx) * sy;
      const double c2 = (q * sx2) * sy2;
      const double tot = c1 + c2;
      double *o = v + 2 * NCOMP;
      o[0] = (kTwoPi * d0) * tot;
      o[1] = (2.355 * fmax(sx, sy)) * pixscale;
      o[2] = (2.355 * fmin(sx, sy)) * pixscale;
      o[3] = (2.355 * fmax(sx2, sy2)) * pixscale;
      o[4] = c1 / tot;
    } else {
      ++nbad;
      for (int p = 0; p < 2 * NCOMP + 5; ++p) v[p] = qnan();
    }
    const size_t at = (size_t)(row0 + r) * W + w;
    for (int p = 0; p < 2 * NCOMP + 5; ++p) store[(size_t)p * N + at] = canon(v[p]);
  }
  if (nbad) atomicAdd(bad, (unsigned long long)nbad);
}

struct Means {
  double m[kMaxQ];
};

// stage 1: block b of plane blockIdx.y reduces samples [b * kChunk, (b + 1) * kChunk) of
// the plane -- a thread its kPer samples in order, the threads by the fixed tree -- into
// part[plane][0..3][b]: the sum of x (pass 0) or of (x - mean)^2 (pass 1) over the samples
// that are not NaN, their count and the extremes of their keys
__global__ __launch_bounds__(kThreads) void phot_reduce_stage1(
    const double *__restrict__ store, long long N, long long n, int pass, Means mean, int nblk,
    double *__restrict__ part) {
  __shared__ double red[kThreads];
  __shared__ unsigned long long redw[kThreads];
  const double *x = store + (size_t)blockIdx.y * N;
  const double m = mean.m[blockIdx.y];
  double s = 0.0;
  unsigned long long cnt = 0, mn = ~0ull, mx = 0ull;
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  for (int j = 0; j < kPer; ++j) {
    const long long i = base + (long long)j * kThreads;
    if (i >= n) break;
    const double v = x[i];
    if (v != v) continue;
    if (pass == 0) {
      s += v;
    } else {
      const double d = v - m;
      s += d * d;
    }
    const unsigned long long k = okey(v);
    ++cnt;
    mn = k < mn ? k : mn;
    mx = k > mx ? k : mx;
  }
  const double ts = block_sum<kThreads>(s, red);
  const unsigned long long tc = block_word<kThreads, WordSum>(cnt, redw);
  const unsigned long long tn = block_word<kThreads, WordMin>(mn, redw);
  const unsigned long long tx = block_word<kThreads, WordMax>(mx, redw);
  if (threadIdx.x == 0) {
    double *p = part + (size_t)blockIdx.y * 4 * nblk + blockIdx.x;
    unsigned long long *pw = reinterpret_cast<unsigned long long *>(p);
    p[0] = ts;
    pw[(size_t)nblk] = tc;
    pw[(size_t)2 * nblk] = tn;
    pw[(size_t)3 * nblk] = tx;
  }
}

// stage 2: one block per plane, the blocks' partials in a fixed order into out[plane][0..3]
__global__ __launch_bounds__(kThreads) void phot_reduce_stage2(const double *__restrict__ part,
                                                               int nblk,
                                                               double *__restrict__ out) {
  __shared__ double red[kThreads];
  __shared__ unsigned long long redw[kThreads];
  const double *p = part + (size_t)blockIdx.x * 4 * nblk;
  const unsigned long long *pw = reinterpret_cast<const unsigned long long *>(p);
  double s = 0.0;
  unsigned long long cnt = 0, mn = ~0ull, mx = 0ull;
  for (int b = threadIdx.x; b < nblk; b += kThreads) {
    s += p[b];
    cnt += pw[(size_t)nblk + b];
    const unsigned long long l = pw[(size_t)2 * nblk + b], h = pw[(size_t)3 * nblk + b];
    mn = l < mn ? l : mn;
    mx = h > mx ? h : mx;
  }
  const double ts = block_sum<kThreads>(s, red);
  const unsigned long long tc = block_word<kThreads, WordSum>(cnt, redw);
  const unsigned long long tn = block_word<kThreads, WordMin>(mn, redw);
  const unsigned long long tx = block_word<kThreads, WordMax>(mx, redw);
  if (threadIdx.x == 0) {
    double *o = out + (size_t)blockIdx.x * 4;
    unsigned long long *ow = reinterpret_cast<unsigned long long *>(o);
    o[0] = ts;
    ow[1] = tc;
    ow[2] = tn;
    ow[3] = tx;
  }
}

struct PlaneSum {
  double sum;
  unsigned long long count, kmin, kmax;
};

// one reduction pass over the n filled samples of every plane into host res[Q]
int reduce(olpe_phot *a, long long n, int pass, const Means &mean, PlaneSum *res) {
  const int nblk = (int)((n + kChunk - 1) / kChunk);
  hipLaunchKernelGGL(phot_reduce_stage1, dim3(nblk, a->Q), dim3(kThreads), 0, a->stream,
                     a->d_store, a->W * a->cap, n, pass, mean, nblk, a->d_part);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(phot_reduce_stage2, dim3(a->Q), dim3(kThreads), 0, a->stream, a->d_part,
                     nblk, a->d_out);
  HIPCHK(hipGetLastError());
  static_assert(sizeof(PlaneSum) == 32, "four words per plane");
  HIPCHK(hipMemcpyAsync(res, a->d_out, (size_t)a->Q * sizeof(PlaneSum), hipMemcpyDeviceToHost,
                        a->stream));
  HIPCHK(hipStreamSynchronize(a->stream));
  return OLPE_OK;
}

// launches the fold of nrows rows on `stream`
int launch_fold(olpe_phot *a, hipStream_t stream, const double *src, long long sw, long long sr,
                long long nrows) {
  const dim3 grid((unsigned)((nrows + kTR - 1) / kTR), (unsigned)((a->W + kTW - 1) / kTW));
  const int rows_inner = sr < sw ? 1 : 0;
  const long long N = a->W * a->cap;
  if (a->variant == 2)
    hipLaunchKernelGGL(phot_fold_kernel<2>, grid, dim3(kThreads), 0, stream, src, sw, sr,
                       rows_inner, a->W, nrows, a->rows, N, a->pixscale, a->d_store, a->d_words);
  else
    hipLaunchKernelGGL(phot_fold_kernel<3>, grid, dim3(kThreads), 0, stream, src, sw, sr,
                       rows_inner, a->W, nrows, a->rows, N, a->pixscale, a->d_store, a->d_words);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_phot_create(int device, int variant, int ps, double pixscale, long long walkers,
                     long long row_cap, olpe_phot **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (variant != 2 && variant != 3) return set_err(OLPE_EINVAL, "variant %d: 2 or 3", variant);
  const int need = variant == 2 ? Cols<2>::first + Cols<2>::n : Cols<3>::first + Cols<3>::n;
  if (ps < need)
    return set_err(OLPE_EINVAL, "PS %d: the %d-source planes read columns up to %d", ps, variant,
                   need - 1);
  if (!isfinite(pixscale)) return set_err(OLPE_EINVAL, "non-finite pixscale");
  int rc;
  if ((rc = store_geometry(walkers, row_cap, kTW))) return rc;
  if ((rc = open_device(device))) return rc;
  olpe_phot *a = new olpe_phot;
  a->variant = variant;
  a->ps = ps;
  a->Q = 2 * (variant - 1) + 5;
  a->pixscale = pixscale;
  a->W = walkers;
  a->cap = row_cap;
  const size_t N = (size_t)walkers * row_cap;
  const size_t nblk = (N + kChunk - 1) / kChunk;
  rc = fold_open(a, device);
  if (!rc) rc = alloc((void **)&a->d_store, N * a->Q * 8, "the photometry sample store");
  if (!rc) rc = alloc((void **)&a->d_part, nblk * 4 * a->Q * 8, "the reduction partials");
  if (!rc) rc = alloc((void **)&a->d_out, (size_t)kMaxQ * 4 * 8, "the reduction results");
  if (!rc) rc = alloc((void **)&a->d_words, 2 * 8, "the photometry words");
  if (!rc) rc = alloc((void **)&a->d_hist, kSelBins * 8, "the select histogram");
  if (!rc && hipMemset(a->d_words, 0, 2 * 8) != hipSuccess)
    rc = set_err(OLPE_EHIP, "hipMemset failed");
  if (rc) {
    olpe_phot_destroy(a);
    return rc;
  }
  *out = a;
  return OLPE_OK;
}

void olpe_phot_destroy(olpe_phot *a) {
  if (!a) return;
  fold_close(a, {a->d_store, a->d_part, a->d_out, a->d_words, a->d_hist, a->d_stage});
  delete a;
}

int olpe_phot_fold_ctx(olpe_phot *a, olpe_ctx *c, int row_step) {
  if (!a || !c) return set_err(OLPE_EINVAL, "NULL argument");
  if (row_step <= 0) return set_err(OLPE_EINVAL, "row_step %d: must be > 0", row_step);
  if (c->device != a->device || c->W != a->W || c->ps != a->ps || c->nsrc != a->variant)
    return set_err(OLPE_EINVAL, "context of device %d, %d walkers, PS %d, %d sources; photometry "
                   "of device %d, %lld walkers, PS %d, %d sources", c->device, c->W, c->ps,
                   c->nsrc, a->device, a->W, a->ps, a->variant);
  int rc;
  if ((rc = fold_check(a, c))) return rc;
  // rows 0, row_step, ... of the chain [W][nrec][PS]: indexing only
  const long long nr = (c->chain_rows + row_step - 1) / row_step;
  if ((rc = store_room(a, nr))) return rc;
  HIPCHK(hipSetDevice(a->device));
  if ((rc = fold_run(a, c, nr > 0, [&](hipStream_t s) {
         return launch_fold(a, s, c->d_chain, c->chain_rows * c->ps, (long long)row_step * c->ps,
                            nr);
       })))
    return rc;
  a->rows += nr;
  return OLPE_OK;
}

int olpe_phot_fold_rows(olpe_phot *a, const double *rows, long long nrows) {
  if (!a || nrows < 0 || (nrows > 0 && !rows)) return set_err(OLPE_EINVAL, "bad argument");
  int rc;
  if ((rc = store_room(a, nrows))) return rc;
  if (nrows == 0) return OLPE_OK;
  // whole rows travel, [rows][W][PS]
  const long long per_row = a->W * a->ps;
  return store_upload(
      a, nrows, per_row, [&](long long r0, long long) { return rows + (size_t)r0 * per_row; },
      [&](long long nr) { return launch_fold(a, a->stream, a->d_stage, a->ps, per_row, nr); });
}

int olpe_phot_rows(olpe_phot *a, long long *rows) { return store_rows(a, rows); }

int olpe_phot_unusable(olpe_phot *a, long long *n) {
  if (!a || !n) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(a->device));
  int rc;
  if ((rc = drain(a))) return rc;
  unsigned long long bad = 0;
  HIPCHK(hipMemcpy(&bad, a->d_words, 8, hipMemcpyDeviceToHost));
  *n = (long long)bad;
  return OLPE_OK;
}

int olpe_phot_finalize(olpe_phot *a, const double *probs, int nprobs, double *out) {
  if (!a || !out || nprobs < 0 || (nprobs > 0 && !probs))
    return set_err(OLPE_EINVAL, "bad argument");
  if (nprobs > kSelMaxRanks) return set_err(OLPE_EINVAL, "%d probabilities: at most %d", nprobs,
                                            kSelMaxRanks);
  for (int j = 0; j < nprobs; ++j)
    if (!(probs[j] >= 0.0 && probs[j] <= 1.0))
      return set_err(OLPE_EINVAL, "probability %g outside [0, 1]", probs[j]);
  if (a->rows == 0) return set_err(OLPE_ESTATE, "no rows folded");
  HIPCHK(hipSetDevice(a->device));
  int rc;
  if ((rc = wait_pending(a))) return rc;
  const long long n = a->rows * a->W;
  const int len = OLPE_PHOT_LEN(nprobs);
  const double nan_ = nan("");
  Means mean = {};
  PlaneSum s1[kMaxQ], s2[kMaxQ];
  if ((rc = reduce(a, n, 0, mean, s1))) return rc;
  for (int q = 0; q < a->Q; ++q)
    mean.m[q] = s1[q].count ? s1[q].sum / (double)s1[q].count : 0.0;
  if ((rc = reduce(a, n, 1, mean, s2))) return rc;
  // the ranks in ascending order of the probabilities, floor((n - 1) p) each
  std::vector<int> order(nprobs);
  for (int j = 0; j < nprobs; ++j) order[j] = j;
  std::sort(order.begin(), order.end(), [&](int x, int y) { return probs[x] < probs[y]; });
  for (int q = 0; q < a->Q; ++q) {
    double *o = out + (size_t)q * len;
    const unsigned long long cnt = s1[q].count;
    o[0] = (double)cnt;
    for (int i = 1; i < len; ++i) o[i] = nan_;
    o[5] = 0.0;
    if (cnt == 0) continue;
    const double fn = (double)cnt;
    o[3] = okey_inv(s1[q].kmin);
    o[4] = okey_inv(s1[q].kmax);
    if (s1[q].kmin == s1[q].kmax) {      // one value throughout: it is the mean, exactly
      o[1] = o[3];
      o[2] = 0.0;
    } else {
      o[1] = mean.m[q];
      o[2] = sqrt(s2[q].sum / fn);
    }
    if (nprobs == 0) continue;
    double vi[kSelMaxRanks];                               // np.percentile's virtual indices
    unsigned long long lo[kSelMaxRanks], hi[kSelMaxRanks];
    for (int i = 0; i < nprobs; ++i) vi[i] = (fn - 1.0) * probs[order[i]];
    int passes = 0;
    if ((rc = select_brackets(a->stream, a->d_hist, a->d_words + 1, store_plane(a, q), n, cnt,
                              s1[q].kmin, s1[q].kmax, vi, nprobs, lo, hi, &passes)))
      return rc;
    for (int i = 0; i < nprobs; ++i) {
      o[6 + 2 * order[i]] = okey_inv(lo[i]);
      o[7 + 2 * order[i]] = okey_inv(hi[i]);
    }
    o[5] = (double)passes;
  }
  return OLPE_OK;
}

int olpe_phot_samples(olpe_phot *a, int plane, double *out) {
  if (!a || !out) return set_err(OLPE_EINVAL, "NULL argument");
  if (plane < 0 || plane >= a->Q) return set_err(OLPE_EINVAL, "plane %d of %d", plane, a->Q);
  HIPCHK(hipSetDevice(a->device));
  int rc;
  if ((rc = drain(a))) return rc;
  return store_read(a, plane, out);
}

int olpe_phot_reset(olpe_phot *a) {
  if (!a) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(a->device));
  int rc;
  if ((rc = drain(a))) return rc;
  HIPCHK(hipMemset(a->d_words, 0, 2 * 8));
  a->rows = 0;
  fold_forget(a);
  return OLPE_OK;
}

}  // extern "C"
