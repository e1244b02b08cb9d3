// olpe_astrom.hip -- separation / position-angle posteriors of the recorded chains, on the
// device (the astrometry step 3 exists for: apf_step3.py:211-256, :283-343, :401-450;
// 3body/apf_step3_3body.py:247-288, :315-390, :450-518).
//
// An olpe_astrom belongs to a device, not to a sampler context.  It holds the per-pair
// configuration, the optional NIRC2 distortion tables (f64, on the device) and a store of
// derived samples: per pair two arrays [cap][W] (row-major over the rows, the walkers
// inner -- the order of step3.load_chains), sample (row r, walker w) at r * W + w.
//   * the fold kernel turns a launch's rows into (sep, pa) at their global positions --
//     one block per (row, 256 walkers), which also leaves the block's sums of the
//     de-distorted positions in a partials array keyed by (row, walker group): neither
//     depends on how the rows were split over folds;
//   * finalize reduces the filled prefix of the store in a fixed order (blocks of
//     kChunk samples, a fixed tree inside each, the blocks' partials by one block):
//     mean(pa), then -- the host having taken the reference's scalar decisions -- the
//     per-sample refraction correction in place, the means and the squared deviations
//     (two passes, as np.std), and the exact medians by radix select on order-preserving
//     64-bit keys (olpe_select.h, shared with olpe_phot.hip).
// Device libm's atan2 / tan / atan / sin / cos differ from the host's by a few ulp: the
// per-sample values are compared to a tolerance, the select exactly.
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

using namespace olpe;

// the store holds [npairs][2] planes: sep and pa per pair
struct olpe_astrom : SampleStore {
  int npairs = 1;
  int cols[2][4] = {};        // per pair: x / y of the primary, x / y of the companion
  bool have_tab = false;
  int tny = 0, tnx = 0, xdiff = 0, ydiff = 0;
  double pixscale = 0, rotation_angle = 0, rotcorr = 0;
  int use_rotcorr = 0;
  bool finalized = false;
  double *d_xd = nullptr, *d_yd = nullptr;
  double *d_pos = nullptr;    // [cap * G][npairs][4] block sums of the positions
  // d_part [4][nblk], d_out [8], d_words [1..4] min / max keys of sep and pa, [5] next key
};

namespace {

constexpr int kThreads = 256;
constexpr int kPer = 16;                       // samples per thread of a reduction block
constexpr long long kChunk = kThreads * kPer;  // samples per reduction block
constexpr double kDeg2Rad = M_PI / 180.0;      // np.radians / np.degrees multiply by these
constexpr double kRad2Deg = 180.0 / M_PI;

struct FoldCfg {
  int variant, npairs, cols[2][4];
  int have_tab, tny, tnx, xdiff, ydiff;
  double pixscale, rotation_angle, rotcorr;
  int use_rotcorr;
  const double *xd, *yd;
};

// x + 1 (:211-214), np.int_ (:234-237), + diff (:244-247); false if the position cannot
// index the table (non-finite, or an index outside it): nothing is loaded then
__device__ __forceinline__ bool table_index(double x1, int diff, int n, int have_tab, int &idx) {
  idx = 0;
  if (!isfinite(x1)) return false;
  if (!have_tab) return true;
  if (!(fabs(x1) < 1073741824.0)) return false;   // beyond any table (and any int)
  const int i = (int)x1 + diff;                   // truncation toward zero, as np.int_
  if (i < 0 || i >= n) return false;
  idx = i;
  return true;
}

// One block per (row, 256 walkers).  src element (row r, walker w, column c) at
// w * sw + r * sr + c.  Sample (row0 + r, w) goes to row-major position (row0 + r) * W + w.
__global__ __launch_bounds__(kThreads) void astrom_fold_kernel(
    const double *__restrict__ src, long long sw, long long sr, FoldCfg cfg, long long W,
    long long row0, long long N, double *__restrict__ store, double *__restrict__ pos,
    unsigned long long *__restrict__ bad) {
  __shared__ double red[kThreads];
  const long long r = blockIdx.x;
  const long long w = (long long)blockIdx.y * kThreads + threadIdx.x;
  const bool act = w < W;
  const double *x = src + (act ? w * sw + r * sr : 0);
  const size_t at = (size_t)(row0 + r) * W + (act ? w : 0);
  const size_t pblk = ((size_t)(row0 + r) * gridDim.y + blockIdx.y) * cfg.npairs * 4;
  unsigned nbad = 0;
  for (int p = 0; p < cfg.npairs; ++p) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};           // de-distorted xs, ys, xc, yc
    double sep = nan(""), pa = nan("");
    if (act) {
      bool ok = true;
      int ix[2], iy[2];
      for (int s = 0; s < 2; ++s) {
        v[2 * s] = x[cfg.cols[p][2 * s]] + 1;     // :211-214
        v[2 * s + 1] = x[cfg.cols[p][2 * s + 1]] + 1;
        ok = table_index(v[2 * s], cfg.xdiff, cfg.tnx, cfg.have_tab, ix[s]) && ok;
        ok = table_index(v[2 * s + 1], cfg.ydiff, cfg.tny, cfg.have_tab, iy[s]) && ok;
      }
      if (ok) {
        if (cfg.have_tab) {
          for (int s = 0; s < 2; ++s) {           // :250-253 (indices clamped above)
            const size_t t = (size_t)iy[s] * cfg.tnx + ix[s];
            v[2 * s] = v[2 * s] + cfg.xd[t];
            v[2 * s + 1] = v[2 * s + 1] + cfg.yd[t];
          }
        }
        const double dy = v[3] - v[1], dx = v[2] - v[0];      // :255-256
        sep = sqrt(dy * dy + dx * dx) * cfg.pixscale;         // :283-286
        pa = atan2(-dx, dy) * kRad2Deg;                       // :290-291
        if (cfg.variant == 3) {                               // 3body :334, np.remainder
          if (pa == 0.0) pa = 0.0;
          else if (pa < 0.0) pa = pa + 360.0;
        }
        pa = pa + cfg.rotation_angle;                         // :304
        if (cfg.use_rotcorr) pa = pa + cfg.rotcorr;           // :337
      } else {
        ++nbad;
        v[0] = v[1] = v[2] = v[3] = 0.0;
      }
      store[(size_t)(2 * p) * N + at] = sep;
      store[(size_t)(2 * p + 1) * N + at] = pa;
    }
    for (int k = 0; k < 4; ++k) {
      const double s = block_sum<kThreads>(v[k], red);
      if (threadIdx.x == 0) pos[pblk + p * 4 + k] = s;
    }
  }
  if (nbad) atomicAdd(bad, (unsigned long long)nbad);
}

struct CorrCfg {
  int variant;
  int add360;      // :340
  int below;       // :402
  int off_mode;    // 0: nothing added, 1: + off, 2: + 180 per sample where < 0 (3body :462)
  double off;
  double deltaR, parantel;
};

// the refraction correction per sample, in the reference's operation order (:340-341,
// :401-430; 3body :450-486): (sep, pa) -> (sep_corrected, pa_angle) in place, and the
// extremes of both arrays' keys
__global__ __launch_bounds__(kThreads) void astrom_correct_kernel(
    double *__restrict__ sepv, double *__restrict__ pav, long long n, CorrCfg c,
    unsigned long long *__restrict__ words) {
  __shared__ unsigned long long red[kThreads];
  unsigned long long mn[2] = {~0ull, ~0ull}, mx[2] = {0ull, 0ull};
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n;
       i += (long long)gridDim.x * kThreads) {
    const double sep = sepv[i];
    double pa = pav[i];
    if (c.add360) pa = pa + 360.;
    const double t = pa - c.parantel;
    const double a = c.below ? (180. - t) * kDeg2Rad : t * kDeg2Rad;
    const double sep_c = sep + c.deltaR * cos(a);
    const double pa_mas = (c.variant == 3 ? sep_c : sep) * tan(pa * kDeg2Rad);
    const double pa_mas_c = pa_mas + c.deltaR * sin(a);
    double ang = atan(pa_mas_c / sep_c) * kRad2Deg;
    if (c.off_mode == 1) ang = ang + c.off;
    else if (c.off_mode == 2 && ang < 0) ang = ang + 180.;
    sepv[i] = sep_c;
    pav[i] = ang;
    const unsigned long long k0 = okey(sep_c), k1 = okey(ang);
    mn[0] = k0 < mn[0] ? k0 : mn[0];
    mx[0] = k0 > mx[0] ? k0 : mx[0];
    mn[1] = k1 < mn[1] ? k1 : mn[1];
    mx[1] = k1 > mx[1] ? k1 : mx[1];
  }
  for (int q = 0; q < 2; ++q) {
    mn[q] = block_word<kThreads, WordMin>(mn[q], red);
    mx[q] = block_word<kThreads, WordMax>(mx[q], red);
  }
  if (threadIdx.x == 0) {      // integer min / max: the same whatever the order
    atomicMin(&words[0], mn[0]);
    atomicMax(&words[1], mx[0]);
    atomicMin(&words[2], mn[1]);
    atomicMax(&words[3], mx[1]);
  }
}

struct RedCfg {
  int kind;        // 0: pa + add; 1: sep, pa, RA, Dec; 2: their squared deviations;
                   // 3: a[i * stride]
  int variant;
  long long stride;
  double add;
  double m[4];
};

__device__ __forceinline__ void radec(int variant, double sep, double pa, double &ra,
                                      double &dec) {
  const double a = pa * kDeg2Rad;
  if (variant == 3) {          // 3body :508-509
    ra = sep * sin(a);
    dec = sep * cos(a);
  } else {                     // :446-447
    ra = sep * cos(a);
    dec = sep * sin(a);
  }
}

// stage 1: block b sums samples [b * kChunk, (b + 1) * kChunk) -- a thread its kPer
// samples in order, the threads by the fixed tree -- into part[v][b]
__global__ __launch_bounds__(kThreads) void astrom_reduce_stage1(
    const double *__restrict__ a, const double *__restrict__ b, long long n, RedCfg c, int nblk,
    double *__restrict__ part) {
  __shared__ double red[kThreads];
  const int nv = (c.kind == 1 || c.kind == 2) ? 4 : 1;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const long long base = (long long)blockIdx.x * kChunk + threadIdx.x;
  for (int j = 0; j < kPer; ++j) {
    const long long i = base + (long long)j * kThreads;
    if (i >= n) break;
    if (c.kind == 0) {
      s[0] += c.add != 0.0 ? a[i] + c.add : a[i];
    } else if (c.kind == 3) {
      s[0] += a[i * c.stride];
    } else {
      double v[4];
      v[0] = a[i];
      v[1] = b[i];
      radec(c.variant, v[0], v[1], v[2], v[3]);
      for (int k = 0; k < 4; ++k) {
        if (c.kind == 1) {
          s[k] += v[k];
        } else {
          const double d = v[k] - c.m[k];
          s[k] += d * d;
        }
      }
    }
  }
  for (int k = 0; k < nv; ++k) {
    const double t = block_sum<kThreads>(s[k], red);
    if (threadIdx.x == 0) part[(size_t)k * nblk + blockIdx.x] = t;
  }
}

// sums of `nv` values over n samples into host out[nv]: stage 2 is one block per value, the
// blocks' partials in a fixed order
int reduce(olpe_astrom *a, const double *x, const double *y, long long n, const RedCfg &c,
           int nv, double *out) {
  const int nblk = (int)((n + kChunk - 1) / kChunk);
  hipLaunchKernelGGL(astrom_reduce_stage1, dim3(nblk), dim3(kThreads), 0, a->stream, x, y, n, c,
                     nblk, a->d_part);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(reduce_stage2_kernel<kThreads>, dim3(nv), dim3(kThreads), 0, a->stream,
                     a->d_part, nblk, a->d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, a->d_out, nv * sizeof(double), hipMemcpyDeviceToHost, a->stream));
  HIPCHK(hipStreamSynchronize(a->stream));
  return OLPE_OK;
}

// np.median of x[0..n): the bracket at the virtual index (n - 1) / 2 (exact in a double: n <=
// 2^40) by radix select below the common prefix of the keys (kmin / kmax: their extremes),
// and where n is even the mean of the pair (olpe_select.h)
int median(olpe_astrom *a, const double *x, long long n, unsigned long long kmin,
           unsigned long long kmax, double *out) {
  const double mid = (double)(n - 1) * 0.5;
  unsigned long long k1, k2;
  int rc;
  if ((rc = select_brackets(a->stream, a->d_hist, a->d_words + 5, x, n, (unsigned long long)n,
                            kmin, kmax, &mid, 1, &k1, &k2, nullptr)))
    return rc;
  const double v1 = okey_inv(k1), v2 = okey_inv(k2);
  *out = n % 2 ? v1 : (v1 + v2) / 2.0;                     // np.mean of the middle pair
  return OLPE_OK;
}

FoldCfg fold_cfg(const olpe_astrom *a) {
  FoldCfg f;
  f.variant = a->variant;
  f.npairs = a->npairs;
  memcpy(f.cols, a->cols, sizeof(f.cols));
  f.have_tab = a->have_tab ? 1 : 0;
  f.tny = a->tny;
  f.tnx = a->tnx;
  f.xdiff = a->xdiff;
  f.ydiff = a->ydiff;
  f.pixscale = a->pixscale;
  f.rotation_angle = a->rotation_angle;
  f.rotcorr = a->rotcorr;
  f.use_rotcorr = a->use_rotcorr;
  f.xd = a->d_xd;
  f.yd = a->d_yd;
  return f;
}

long long groups(const olpe_astrom *a) { return (a->W + kThreads - 1) / kThreads; }

// launches the fold of nrows rows on `stream`
int launch_fold(olpe_astrom *a, hipStream_t stream, const double *src, long long sw,
                long long sr, const FoldCfg &f, long long nrows) {
  hipLaunchKernelGGL(astrom_fold_kernel, dim3((unsigned)nrows, (unsigned)groups(a)),
                     dim3(kThreads), 0, stream, src, sw, sr, f, a->W, a->rows, a->W * a->cap,
                     a->d_store, a->d_pos, a->d_words);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_astrom_create(int device, int variant, int ps, const int *pair_cols, int npairs,
                       const double *x_dist, const double *y_dist, int tab_ny, int tab_nx,
                       int xdiff, int ydiff, double pixscale, double rotation_angle,
                       double rotcorr, int use_rotcorr, long long walkers, long long row_cap,
                       olpe_astrom **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (variant != 2 && variant != 3) return set_err(OLPE_EINVAL, "variant %d: 2 or 3", variant);
  if (npairs != (variant == 2 ? 1 : 2))
    return set_err(OLPE_EINVAL, "variant %d has %d pair(s), not %d", variant, variant - 1, npairs);
  if (!pair_cols || ps < 4) return set_err(OLPE_EINVAL, "NULL pair columns or PS %d < 4", ps);
  for (int i = 0; i < 4 * npairs; ++i)
    if (pair_cols[i] < 0 || pair_cols[i] >= ps)
      return set_err(OLPE_EINVAL, "pair column %d outside [0, %d)", pair_cols[i], ps);
  if ((x_dist == nullptr) != (y_dist == nullptr))
    return set_err(OLPE_EINVAL, "one distortion table without the other");
  if (x_dist && (tab_ny < 1 || tab_nx < 1 || tab_ny > 65536 || tab_nx > 65536))
    return set_err(OLPE_EINVAL, "distortion tables of %d x %d", tab_ny, tab_nx);
  if (!isfinite(pixscale) || !isfinite(rotation_angle) || (use_rotcorr && !isfinite(rotcorr)))
    return set_err(OLPE_EINVAL, "non-finite pixscale / rotation_angle / rotcorr");
  int rc;
  if ((rc = store_geometry(walkers, row_cap, kThreads))) return rc;
  if ((rc = open_device(device))) return rc;
  olpe_astrom *a = new olpe_astrom;
  a->variant = variant;
  a->ps = ps;
  a->npairs = npairs;
  for (int p = 0; p < npairs; ++p)
    for (int k = 0; k < 4; ++k) a->cols[p][k] = pair_cols[4 * p + k];
  a->have_tab = x_dist != nullptr;
  a->tny = tab_ny;
  a->tnx = tab_nx;
  a->xdiff = xdiff;
  a->ydiff = ydiff;
  a->pixscale = pixscale;
  a->rotation_angle = rotation_angle;
  a->rotcorr = rotcorr;
  a->use_rotcorr = use_rotcorr ? 1 : 0;
  a->W = walkers;
  a->cap = row_cap;
  const size_t N = (size_t)walkers * row_cap;
  const size_t nblk = (N + kChunk - 1) / kChunk;
  const size_t npos = (size_t)row_cap * groups(a) * npairs * 4;
  rc = fold_open(a, device);
  if (!rc) rc = alloc((void **)&a->d_store, N * 2 * npairs * 8, "the astrometry sample store");
  if (!rc) rc = alloc((void **)&a->d_pos, npos * 8, "the position partials");
  if (!rc) rc = alloc((void **)&a->d_part, std::max<size_t>(nblk, npos / kChunk + 1) * 4 * 8,
                      "the reduction partials");
  if (!rc) rc = alloc((void **)&a->d_out, 8 * 8, "the reduction results");
  if (!rc) rc = alloc((void **)&a->d_words, 8 * 8, "the astrometry words");
  if (!rc) rc = alloc((void **)&a->d_hist, kSelBins * 8, "the select histogram");
  if (!rc && a->have_tab) {
    const size_t tb = (size_t)tab_ny * tab_nx * 8;
    rc = alloc((void **)&a->d_xd, tb, "the X distortion table");
    if (!rc) rc = alloc((void **)&a->d_yd, tb, "the Y distortion table");
    if (!rc && (hipMemcpy(a->d_xd, x_dist, tb, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(a->d_yd, y_dist, tb, hipMemcpyHostToDevice) != hipSuccess))
      rc = set_err(OLPE_EHIP, "distortion table upload failed");
  }
  if (!rc && hipMemset(a->d_words, 0, 8 * 8) != hipSuccess)
    rc = set_err(OLPE_EHIP, "hipMemset failed");
  if (rc) {
    olpe_astrom_destroy(a);
    return rc;
  }
  *out = a;
  return OLPE_OK;
}

void olpe_astrom_destroy(olpe_astrom *a) {
  if (!a) return;
  fold_close(a, {a->d_xd, a->d_yd, a->d_store, a->d_pos, a->d_part, a->d_out, a->d_words,
                 a->d_hist, a->d_stage});
  delete a;
}

int olpe_astrom_fold_ctx(olpe_astrom *a, olpe_ctx *c) {
  if (!a || !c) return set_err(OLPE_EINVAL, "NULL argument");
  if (c->device != a->device || c->W != a->W || c->ps != a->ps)
    return set_err(OLPE_EINVAL, "context of device %d, %d walkers, PS %d; astrometry of device "
                   "%d, %lld walkers, PS %d", c->device, c->W, c->ps, a->device, a->W, a->ps);
  if (a->finalized) return set_err(OLPE_ESTATE, "fold after finalize");
  int rc;
  if ((rc = fold_check(a, c))) return rc;
  const long long nrec = c->chain_rows;
  if ((rc = store_room(a, nrec))) return rc;
  HIPCHK(hipSetDevice(a->device));
  if ((rc = fold_run(a, c, nrec > 0, [&](hipStream_t s) {
         return launch_fold(a, s, c->d_chain, nrec * c->ps, c->ps, fold_cfg(a), nrec);
       })))
    return rc;
  a->rows += nrec;
  return OLPE_OK;
}

int olpe_astrom_fold_rows(olpe_astrom *a, const double *rows, long long nrows) {
  if (!a || nrows < 0 || (nrows > 0 && !rows)) return set_err(OLPE_EINVAL, "bad argument");
  if (a->finalized) return set_err(OLPE_ESTATE, "fold after finalize");
  int rc;
  if ((rc = store_room(a, nrows))) return rc;
  if (nrows == 0) return OLPE_OK;
  // only the position columns travel: [rows][W][nu], the pairs' columns renumbered
  int uniq[8], nu = 0;
  FoldCfg f = fold_cfg(a);
  for (int p = 0; p < a->npairs; ++p)
    for (int k = 0; k < 4; ++k) {
      int j = 0;
      while (j < nu && uniq[j] != a->cols[p][k]) ++j;
      if (j == nu) uniq[nu++] = a->cols[p][k];
      f.cols[p][k] = j;
    }
  const long long per_row = a->W * nu;
  std::vector<double> pack;
  return store_upload(
      a, nrows, per_row,
      [&](long long r0, long long nr) {
        const double *src = rows + (size_t)r0 * a->W * a->ps;
        pack.resize((size_t)(nr * per_row));     // the first piece is the largest
        for (long long i = 0; i < nr * a->W; ++i)
          for (int j = 0; j < nu; ++j) pack[(size_t)i * nu + j] = src[(size_t)i * a->ps + uniq[j]];
        return pack.data();
      },
      [&](long long nr) { return launch_fold(a, a->stream, a->d_stage, nu, per_row, f, nr); });
}

int olpe_astrom_finalize(olpe_astrom *a, double delta_r, double parantel, double *out) {
  if (!a || !out) return set_err(OLPE_EINVAL, "NULL argument");
  if (!isfinite(delta_r) || !isfinite(parantel))
    return set_err(OLPE_EINVAL, "non-finite deltaR / parantel");
  if (a->finalized) return set_err(OLPE_ESTATE, "finalize called twice (the store holds the "
                                   "corrected samples)");
  if (a->rows == 0) return set_err(OLPE_ESTATE, "no rows folded");
  HIPCHK(hipSetDevice(a->device));
  int rc;
  if ((rc = wait_pending(a))) return rc;
  unsigned long long bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, a->d_words, 8, hipMemcpyDeviceToHost, a->stream));
  HIPCHK(hipStreamSynchronize(a->stream));
  if (bad)
    return set_err(OLPE_EINVAL, "%llu sample(s) with a non-finite position or a distortion-table "
                   "index outside the table", bad);
  const long long n = a->rows * a->W;
  const double fn = (double)n;
  const long long nposblk = a->rows * groups(a);
  for (int p = 0; p < a->npairs; ++p) {
    double *o = out + (size_t)p * OLPE_ASTROM_LEN;
    double *sep = store_plane(a, 2 * p), *pa = store_plane(a, 2 * p + 1);
    RedCfg r = {};
    r.variant = a->variant;
    // means of the de-distorted positions (reported; they feed nothing else)
    for (int k = 0; k < 4; ++k) {
      r.kind = 3;
      r.stride = (long long)a->npairs * 4;
      double s;
      if ((rc = reduce(a, a->d_pos + p * 4 + k, nullptr, nposblk, r, 1, &s))) return rc;
      o[12 + k] = s / fn;
    }
    // mean(pa) and the reference's scalar decisions
    r.kind = 0;
    r.add = 0.0;
    double s;
    if ((rc = reduce(a, pa, nullptr, n, r, 1, &s))) return rc;
    double mean_pa = s / fn;
    CorrCfg c = {};
    c.variant = a->variant;
    c.deltaR = delta_r;
    c.parantel = parantel;
    if (mean_pa < 0) {                                      // :340-341
      c.add360 = 1;
      r.add = 360.;
      if ((rc = reduce(a, pa, nullptr, n, r, 1, &s))) return rc;
      mean_pa = s / fn;
    }
    const double pop = mean_pa - parantel;                  // :401
    int branch;
    if (pop >= 90. && pop <= 270.) {                        // :402
      c.below = 1;
      if (a->variant == 3) {                                // 3body :462
        c.off_mode = 2;
        branch = OLPE_ASTROM_BELOW_PER_SAMPLE;
      } else if (mean_pa >= 90.) {                          // :412-415
        c.off_mode = 1;
        c.off = 180.;
        branch = OLPE_ASTROM_BELOW_180;
      } else {
        branch = OLPE_ASTROM_BELOW_0;
      }
    } else {
      // :425 tests pop > 270 twice; 3body :481 tests mean(pa) > 270 second
      if (pop > 270. && (a->variant == 2 || mean_pa > 270)) {
        c.off_mode = 1;
        c.off = 360.;
        branch = OLPE_ASTROM_ABOVE_360;
      } else if (pop > 270. && mean_pa < 270) {             // :427, 3body :483
        c.off_mode = 1;
        c.off = 180.;
        branch = OLPE_ASTROM_ABOVE_180;
      } else {
        branch = OLPE_ASTROM_ABOVE_0;
      }
    }
    const unsigned long long init[4] = {~0ull, 0ull, ~0ull, 0ull};
    HIPCHK(hipMemcpyAsync(a->d_words + 1, init, sizeof(init), hipMemcpyHostToDevice, a->stream));
    const unsigned cgrid = (unsigned)std::min<long long>((n + kThreads - 1) / kThreads, 4096);
    hipLaunchKernelGGL(astrom_correct_kernel, dim3(cgrid), dim3(kThreads), 0, a->stream, sep, pa,
                       n, c, a->d_words + 1);
    HIPCHK(hipGetLastError());
    unsigned long long ext[4];
    HIPCHK(hipMemcpyAsync(ext, a->d_words + 1, sizeof(ext), hipMemcpyDeviceToHost, a->stream));
    HIPCHK(hipStreamSynchronize(a->stream));
    // np.std: the mean, then the mean squared deviation about it (:436-437, :449-450)
    double m[4], q[4];
    r.kind = 1;
    if ((rc = reduce(a, sep, pa, n, r, 4, m))) return rc;
    for (int k = 0; k < 4; ++k) r.m[k] = m[k] = m[k] / fn;
    r.kind = 2;
    if ((rc = reduce(a, sep, pa, n, r, 4, q))) return rc;
    if ((rc = median(a, sep, n, ext[0], ext[1], &o[0]))) return rc;
    if ((rc = median(a, pa, n, ext[2], ext[3], &o[2]))) return rc;
    o[1] = sqrt(q[0] / fn);
    o[3] = sqrt(q[1] / fn);
    o[4] = a->variant == 3 ? m[2] : -m[2];                  // :449; 3body :511
    o[5] = sqrt(q[2] / fn);
    o[6] = m[3];
    o[7] = sqrt(q[3] / fn);
    o[8] = mean_pa;
    o[9] = (double)branch;
    o[10] = fn;
    o[11] = (double)c.add360;
  }
  a->finalized = true;
  return OLPE_OK;
}

int olpe_astrom_rows(olpe_astrom *a, long long *rows) { return store_rows(a, rows); }

int olpe_astrom_samples(olpe_astrom *a, int pair, double *out) {
  if (!a || !out) return set_err(OLPE_EINVAL, "NULL argument");
  if (pair < 0 || pair >= a->npairs) return set_err(OLPE_EINVAL, "pair %d of %d", pair, a->npairs);
  if (!a->finalized) return set_err(OLPE_ESTATE, "samples before finalize");
  HIPCHK(hipSetDevice(a->device));
  HIPCHK(hipStreamSynchronize(a->stream));
  int rc;
  if ((rc = store_read(a, 2 * pair, out))) return rc;
  return store_read(a, 2 * pair + 1, out + (size_t)a->rows * a->W);
}

}  // extern "C"
