// olpe_acf.hip -- integrated autocorrelation times of the recorded chains: the numbers
// behind the reference's chain plot (apf_step3.py:582-601 draws every walker's trace of
// every parameter; additional_burnin, accept_min and the record stride are then chosen by
// eye).  An olpe_acf keeps, per column c, the pooled biased lag sums
//     C[c][k] = sum over series  sum_{t=0}^{N-k-1} y[t] y[t+k],   k = 0 .. L,
// where a series is one walker's values of one column over one contiguous run of recorded
// rows, p = x[0] its pivot and y[t] = (x[t] - p) - mean_t(x[t] - p).  A lag k >= N adds
// exactly 0.  A series with a non-finite value in any column is left out whole and
// counted.  The state (C, n, series, skipped) is additive; tau and the effective sample
// size are host arithmetic on it (olpefit_amd/autocorr.py).
//
// Three kernels per fold:
//   * acf_stats_kernel, a workgroup per series: the usable flag, and per column the pivot,
//     the mean of x - p and the one lag the fold's lanes do not own, lag L (a strided dot
//     product), every sum in a fixed order.
//   * acf_fold_kernel, lags 0 .. L - 1.  A workgroup owns a group of G columns and a fixed
//     share ("slot") of the (series, time tile) units; a wave owns one column.  Per unit
//     the workgroup stages T + L rows of the deviations y of its columns in LDS,
//     column-major, zero past row N - 1, so the inner loop needs no masks.  A lane owns
//     R = 8 consecutive lags and walks 64 times in blocks of U = 8: 8 broadcast values
//     and 8 new window values (the other 8 of the 16-value window stay in registers), four
//     ds_read_b128 each, feed 64 FMAs: one LDS read instruction per 8 FMAs.  L / 8 lanes
//     cover the lags; for L < 512 the other lanes take other 64-time stretches of the
//     tile, for L > 512 a lane makes two passes.  The accumulators stay in registers over
//     all of a slot's units.  The window's lane stride is 8 doubles (16 banks): row i
//     lives at i + 2 (i >> 3), a stride of 10 doubles = 5 x 16 bytes, which keeps the
//     16-byte alignment and gives the 16 lanes of a ds_read_b128 group 16 distinct
//     quadruples of banks.
//   * acf_reduce_kernel adds the slots' partial sums in slot order (acf_reduce0_kernel the
//     series' lag-L sums and the counters).  No floating-point atomics.  The slots are a
//     function of the input's shape alone, not of the grid or the device: the same call on
//     the same input gives the same bits.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/olpe.h"
#include "olpe_fold.h"
#include "olpe_internal.h"
#include "olpe_reduce.h"

using namespace olpe;

struct olpe_acf : FoldBase {
  int ncols = 0, L = 0;
  int tile_knob = 0;                  // OLPE_ACF_TILE (0 = chosen per fold)
  double *d_C = nullptr;              // [ncols][L + 1]
  unsigned long long *d_cnt = nullptr;  // {n, series, skipped}
  // per-fold work buffers, grown on demand
  double2 *d_stat = nullptr;          // [series][ncols] {pivot, mean}
  double *d_c0 = nullptr;             // [series][ncols] lag L of a series (0 if unusable)
  int *d_use = nullptr;               // [series]
  size_t ser_cap = 0;
  double *d_part = nullptr;           // [slots][ncols][L] lags 0 .. L - 1
  size_t part_cap = 0;
  double *d_stage = nullptr;          // upload staging of fold_rows
  size_t stage_cap = 0;
};

namespace {

constexpr int kMaxCols = 24, kMinLag = 64, kMaxLag = 1024;
constexpr int kR = 8, kU = 8;                      // lags per lane, times per block
constexpr int kSub = 64;                           // times a lane walks per stretch
constexpr int kMaxTile = 512;                      // rows of a time tile at the most
constexpr int kMaxGroup = 16;                      // columns (waves) per workgroup
constexpr size_t kLdsBudget = 79 * 1024;           // per workgroup: two fit a CU's 160 KiB
constexpr int kMaxSlots = 1024;                    // partial sums per column group
constexpr int kStatThreads = 256;
constexpr size_t kStageBytes = 256ull << 20;       // fold_rows uploads pieces of this size

// row i of a staged column lives at i + 2 (i >> 3)
__host__ __device__ constexpr int skew(int i) { return i + 2 * (i >> 3); }
// doubles per staged column of `rows` rows (a multiple of 64, so skew(rows) is one of 80):
// two more, so that consecutive columns start 4 banks apart -- the staging stores of a wave
// go to consecutive columns of a few rows and would otherwise all hit one bank
__host__ __device__ constexpr int col_stride(int rows) { return skew(rows) + 2; }

struct FoldArgs {
  const double *x;            // value (series s, row t, column c) at x[s * ws + t * rs + c]
  long long ws, rs;
  long long N;                // rows per series
  int C, L;
  int T, tiles;               // rows per time tile, tiles per series
  int S, S64, TG;             // lag slots L / 8, min(S, 64), time groups per wave
  int G;                      // columns per group
  int cs;                     // doubles per staged column
  long long units, chunk;     // series x tiles, units per slot
  const double2 *stat;
  const int *use;
  double *part;               // [slots][C][L]
};

// A workgroup per series: thread (r, c) sums column c over rows r, r + RP, ...; the RP
// partial sums are added in order of r.
__global__ __launch_bounds__(kStatThreads) void acf_stats_kernel(
    const double *__restrict__ x, long long ws, long long rs, long long N, int C, int L,
    double2 *__restrict__ stat, double *__restrict__ c0, int *__restrict__ use) {
  __shared__ double red[kStatThreads];
  __shared__ double mean[kMaxCols];
  __shared__ int bad;
  const long long s = blockIdx.x;
  const double *xs = x + (size_t)s * ws;
  const int RP = kStatThreads / C;
  const int r = threadIdx.x / C, c = threadIdx.x % C;
  const bool on = r < RP;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const double p = on ? xs[c] : 0.0;
  double sum = 0.0;
  bool fin = true;
  if (on)
#pragma unroll 8
    for (long long t = r; t < N; t += RP) {
      const double v = xs[(size_t)t * rs + c];
      fin = fin && isfinite(v);
      sum += v - p;
    }
  if (!fin) bad = 1;
  red[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x < C) {
    double a = 0.0;
    for (int k = 0; k < RP; ++k) a += red[k * C + threadIdx.x];
    mean[threadIdx.x] = a / (double)N;
  }
  __syncthreads();
  const bool usable = !bad;
  const double m = on ? mean[c] : 0.0;
  sum = 0.0;
  if (on && usable)
#pragma unroll 8
    for (long long t = r; t + L < N; t += RP) {
      const double y0 = (xs[(size_t)t * rs + c] - p) - m;
      const double y1 = (xs[(size_t)(t + L) * rs + c] - p) - m;
      sum = __builtin_fma(y0, y1, sum);
    }
  __syncthreads();
  red[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x < C) {
    double a = 0.0;
    for (int k = 0; k < RP; ++k) a += red[k * C + threadIdx.x];
    c0[(size_t)s * C + threadIdx.x] = usable ? a : 0.0;
    stat[(size_t)s * C + threadIdx.x] = make_double2(p, m);
  }
  if (threadIdx.x == 0) use[s] = usable ? 1 : 0;
}

// 64 times x 8 lags of one lane: col = the staged column, t8 = first time / 8 of the
// broadcast values, m8 = (first time + first lag) / 8 of the window.  Both rows are
// multiples of 8 and skew(8 a + q) = 10 a + skew(q), even for even q: every LDS offset
// below is a constant and every pair of rows read is 16-byte aligned (ds_read_b128).
__device__ __forceinline__ void lane_walk(const double *__restrict__ col, int t8, int m8,
                                          double (&acc)[kR]) {
  const double2 *bp = reinterpret_cast<const double2 *>(col) + 5 * t8;
  const double2 *wp = reinterpret_cast<const double2 *>(col) + 5 * m8;
  double w[kR + kU];
#pragma unroll
  for (int i = 0; i < kR; i += 2) {
    const double2 d = wp[skew(i) / 2];
    w[i] = d.x;
    w[i + 1] = d.y;
  }
#pragma unroll
  for (int blk = 0; blk < kSub / kU; ++blk) {
    double b[kU];
#pragma unroll
    for (int u = 0; u < kU; u += 2) {
      const double2 d = bp[skew(blk * kU + u) / 2];
      b[u] = d.x;
      b[u + 1] = d.y;
    }
#pragma unroll
    for (int i = kR; i < kR + kU; i += 2) {
      const double2 d = wp[skew(blk * kU + i) / 2];
      w[i] = d.x;
      w[i + 1] = d.y;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
#pragma unroll
      for (int r = 0; r < kR; ++r) acc[r] = __builtin_fma(b[u], w[r + u], acc[r]);
#pragma unroll
    for (int i = 0; i < kR; ++i) w[i] = w[i + kU];
  }
}

// NP = passes over the lag slots: 1 for L <= 512, 2 above.  blockDim.x = 64 G.
template <int NP>
__global__ __launch_bounds__(64 * kMaxGroup) void acf_fold_kernel(const FoldArgs a) {
  extern __shared__ double2 sy2[];                 // [G][cs] doubles, 16-byte aligned
  double *sy = reinterpret_cast<double *>(sy2);
  const int c0 = blockIdx.y * a.G;
  const int nc = min(a.G, a.C - c0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = lane % a.S64, tg = lane / a.S64;
  const bool wave_on = wave < nc && tg < a.TG;
  double acc[NP][kR];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < kR; ++r) acc[p][r] = 0.0;
  const double *col = sy + (size_t)wave * a.cs;
  const int nrows = a.T + a.L;
  const bool stager = (int)threadIdx.x < 64 * nc;
  const int scc = stager ? threadIdx.x % nc : 0, srow = threadIdx.x / nc;
  const long long u0 = (long long)blockIdx.x * a.chunk;
  const long long u1 = u0 + a.chunk < a.units ? u0 + a.chunk : a.units;
  for (long long u = u0; u < u1; ++u) {
    const long long s = u / a.tiles;
    if (!a.use[s]) continue;                       // the same for the whole workgroup
    const long long t0 = (u - s * a.tiles) * a.T;
    const double *xs = a.x + (size_t)s * a.ws;
    const double2 *st = a.stat + (size_t)s * a.C + c0;
    __syncthreads();                               // the last unit's walks are done
    // 64 nc threads, thread (r, cc) rows r, r + 64, ...: T + L is a multiple of 64, so
    // every thread makes the same number of trips, with no branch (a row past N - 1
    // reads row N - 1 and stores 0) and the loads of several trips in flight
    if (stager) {
      const double2 pm = st[scc];
      const double *xc = xs + c0 + scc;
      double *dst = sy + (size_t)scc * a.cs;
#pragma unroll 7
      for (int row = srow; row < nrows; row += 64) {
        const long long t = t0 + row;
        const double v = xc[(size_t)(t < a.N ? t : a.N - 1) * a.rs];
        dst[skew(row)] = t < a.N ? (v - pm.x) - pm.y : 0.0;
      }
    }
    __syncthreads();
    if (wave_on) {
      // stretches of 64 times; one that starts past row N - 1 holds zeros only
      for (int sub = tg; sub * kSub < a.T && t0 + (long long)sub * kSub < a.N; sub += a.TG) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          const int sp = p * 64 + slot;
          if (sp < a.S) lane_walk(col, sub * (kSub / 8), sub * (kSub / 8) + sp, acc[p]);
        }
      }
    }
  }
  // the time groups' sums of a lag, added in group order by the first group's lane
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int r = 0; r < kR; ++r) {
      const double mine = acc[p][r];
      double sum = mine;
      for (int g = 1; g < a.TG; ++g) sum += __shfl(mine, (lane + g * a.S64) & 63, 64);
      acc[p][r] = sum;
    }
  if (wave < nc && tg == 0) {
    double *out = a.part + ((size_t)blockIdx.x * a.C + c0 + wave) * a.L;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int sp = p * 64 + slot;
      if (sp < a.S)
#pragma unroll
        for (int r = 0; r < kR; ++r) out[sp * kR + r] = acc[p][r];
    }
  }
}

// C[c][k] += the slots' partial sums in slot order, k = 0 .. L - 1
__global__ __launch_bounds__(256) void acf_reduce_kernel(const double *__restrict__ part,
                                                         int slots, int C, int L,
                                                         double *__restrict__ Cout) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * L) return;
  const int c = i / L, k = i - c * L;
  double sum = 0.0;
  for (int p = 0; p < slots; ++p) sum += part[((size_t)p * C + c) * L + k];
  Cout[(size_t)c * (L + 1) + k] += sum;
}

// A workgroup per column: C[c][L] += the series' lag-L sums (thread i takes series i,
// i + 256, ..., then a fixed tree); workgroup 0 also counts the series.
__global__ __launch_bounds__(256) void acf_reduce0_kernel(
    const double *__restrict__ c0, const int *__restrict__ use, long long nser, long long N,
    int C, int L, double *__restrict__ Cout, unsigned long long *__restrict__ cnt) {
  __shared__ double red[256];
  __shared__ unsigned long long used[256];
  const int c = blockIdx.x;
  double sum = 0.0;
  unsigned long long nu = 0;
  for (long long s = threadIdx.x; s < nser; s += 256) {
    sum += c0[(size_t)s * C + c];
    nu += (unsigned long long)use[s];
  }
  sum = block_sum<256>(sum, red);
  nu = block_word<256, WordSum>(nu, used);
  if (threadIdx.x == 0) {
    Cout[(size_t)c * (L + 1) + L] += sum;
    if (c == 0) {
      cnt[0] += nu * (unsigned long long)N;
      cnt[1] += nu;
      cnt[2] += (unsigned long long)nser - nu;
    }
  }
}

// The time tile, the column groups and the lanes' roles for series of N rows.
// Among the tiles (multiples of 64 rows up to 512) whose columns fit the LDS budget, the
// one that stages the fewest rows per row of work, (T + L) / T x groups; the larger on a tie.
int plan(const olpe_acf *h, long long N, FoldArgs *a) {
  const int C = h->ncols, L = h->L;
  int bestT = 0, bestG = 0;
  double best = 0.0;
  for (int T = kSub; T <= kMaxTile; T += kSub) {
    if (h->tile_knob && T != h->tile_knob) continue;
    const size_t colbytes = (size_t)col_stride(T + L) * 8;
    int G = (int)std::min<size_t>(std::min(C, kMaxGroup), kLdsBudget / colbytes);
    if (G < 1) continue;
    const int groups = (C + G - 1) / G;
    G = (C + groups - 1) / groups;
    const double score = (double)groups * (T + L) / T;
    if (!bestT || score <= best) {
      best = score;
      bestT = T;
      bestG = G;
    }
  }
  if (!bestT) return set_err(OLPE_EINVAL, "no time tile fits the LDS for max_lag %d", L);
  a->C = C;
  a->L = L;
  a->N = N;
  a->T = bestT;
  a->G = bestG;
  a->cs = col_stride(bestT + L);
  a->tiles = (int)((N + bestT - 1) / bestT);
  a->S = L / kR;
  a->S64 = std::min(a->S, 64);
  // time groups: as many as the wave's lanes hold, a divisor of the tile's stretches
  int tg = std::min(64 / a->S64, bestT / kSub);
  while ((bestT / kSub) % tg) --tg;
  a->TG = tg;
  return OLPE_OK;
}

// the kernels over nser series of N rows at d_x, on `stream`
int launch_fold(olpe_acf *h, hipStream_t stream, const double *d_x, long long ws, long long rs,
                long long nser, long long N) {
  FoldArgs a = {};
  int rc;
  if (nser > 0x7fffffffll) return set_err(OLPE_EINVAL, "%lld series in one fold", nser);
  if ((rc = plan(h, N, &a))) return rc;
  const int C = h->ncols, L = h->L;
  a.x = d_x;
  a.ws = ws;
  a.rs = rs;
  a.units = nser * a.tiles;
  long long slots = std::min<long long>(a.units, kMaxSlots);
  a.chunk = (a.units + slots - 1) / slots;
  slots = (a.units + a.chunk - 1) / a.chunk;
  a.stat = h->d_stat;
  a.use = h->d_use;
  a.part = h->d_part;
  hipLaunchKernelGGL(acf_stats_kernel, dim3((unsigned)nser), dim3(kStatThreads), 0, stream, d_x,
                     ws, rs, N, C, L, h->d_stat, h->d_c0, h->d_use);
  HIPCHK(hipGetLastError());
  const int groups = (C + a.G - 1) / a.G;
  const size_t lds = (size_t)a.G * a.cs * 8;
  const dim3 grid((unsigned)slots, (unsigned)groups), block(64 * a.G);
  if (L > 512)
    hipLaunchKernelGGL(acf_fold_kernel<2>, grid, block, lds, stream, a);
  else
    hipLaunchKernelGGL(acf_fold_kernel<1>, grid, block, lds, stream, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(acf_reduce_kernel, dim3((C * L + 255) / 256), dim3(256), 0, stream,
                     h->d_part, (int)slots, C, L, h->d_C);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(acf_reduce0_kernel, dim3(C), dim3(256), 0, stream, h->d_c0, h->d_use, nser,
                     N, C, L, h->d_C, h->d_cnt);
  HIPCHK(hipGetLastError());
  return OLPE_OK;
}

// the work buffers of a fold of nser series (drained first: they may be replaced)
int reserve(olpe_acf *h, long long nser) {
  const size_t C = (size_t)h->ncols;
  if ((size_t)nser > h->ser_cap) {
    int rc;
    if ((rc = drain(h))) return rc;
    void *bufs[] = {h->d_stat, h->d_c0, h->d_use};
    for (void *b : bufs)
      if (b) (void)hipFree(b);
    h->d_stat = nullptr;
    h->d_c0 = nullptr;
    h->d_use = nullptr;
    h->ser_cap = 0;
    if ((rc = alloc((void **)&h->d_stat, (size_t)nser * C * sizeof(double2), "the series' pivots")))
      return rc;
    if ((rc = alloc((void **)&h->d_c0, (size_t)nser * C * 8, "the series' lag-L sums"))) return rc;
    if ((rc = alloc((void **)&h->d_use, (size_t)nser * sizeof(int), "the series' flags")))
      return rc;
    h->ser_cap = (size_t)nser;
  }
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_acf_create(int device, int ncols, int max_lag, olpe_acf **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (ncols < 1 || ncols > kMaxCols)
    return set_err(OLPE_EINVAL, "ncols %d: 1 to %d columns", ncols, kMaxCols);
  if (max_lag < kMinLag || max_lag > kMaxLag || max_lag % 64)
    return set_err(OLPE_EINVAL, "max_lag %d: a multiple of 64 from %d to %d", max_lag, kMinLag,
                   kMaxLag);
  int knob = 0;
  if (const char *t = getenv("OLPE_ACF_TILE")) {
    char *end = nullptr;
    const long v = strtol(t, &end, 10);
    if (!*t || *end || v < kSub || v > kMaxTile || v % kSub)
      return set_err(OLPE_EINVAL, "OLPE_ACF_TILE=%s: a multiple of %d from %d to %d", t, kSub,
                     kSub, kMaxTile);
    if ((size_t)col_stride((int)v + max_lag) * 8 > kLdsBudget)
      return set_err(OLPE_EINVAL, "OLPE_ACF_TILE=%s: one column of %ld + %d rows exceeds the LDS "
                     "budget of %zu bytes", t, v, max_lag, kLdsBudget);
    knob = (int)v;
  }
  int rc;
  if ((rc = open_device(device))) return rc;
  olpe_acf *h = new olpe_acf;
  h->ncols = ncols;
  h->L = max_lag;
  h->tile_knob = knob;
  const size_t cb = (size_t)ncols * (max_lag + 1) * 8;
  // one slot array serves every fold: [kMaxSlots][ncols][L]
  const size_t pb = (size_t)kMaxSlots * ncols * max_lag * 8;
  rc = fold_open(h, device);
  if (!rc && (hipFuncSetAttribute((const void *)acf_fold_kernel<1>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kLdsBudget) != hipSuccess ||
              hipFuncSetAttribute((const void *)acf_fold_kernel<2>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)kLdsBudget) != hipSuccess))
    rc = set_err(OLPE_EHIP, "the fold kernel's LDS size was refused");
  if (!rc) rc = alloc((void **)&h->d_C, cb, "the lag sums");
  if (!rc) rc = alloc((void **)&h->d_cnt, 3 * 8, "the counters");
  if (!rc) rc = alloc((void **)&h->d_part, pb, "the partial lag sums");
  if (!rc) h->part_cap = pb;
  if (!rc && (hipMemset(h->d_C, 0, cb) != hipSuccess || hipMemset(h->d_cnt, 0, 3 * 8) != hipSuccess))
    rc = set_err(OLPE_EHIP, "zeroing the state failed");
  if (rc) {
    olpe_acf_destroy(h);
    return rc;
  }
  *out = h;
  return OLPE_OK;
}

void olpe_acf_destroy(olpe_acf *h) {
  if (!h) return;
  fold_close(h, {h->d_C, h->d_cnt, h->d_stat, h->d_c0, h->d_use, h->d_part, h->d_stage});
  delete h;
}

int olpe_acf_fold_ctx(olpe_acf *h, olpe_ctx *c) {
  if (!h || !c) return set_err(OLPE_EINVAL, "NULL argument");
  if (c->device != h->device || c->ps != h->ncols)
    return set_err(OLPE_EINVAL, "context of device %d, PS %d; autocorrelation of device %d, %d "
                   "columns", c->device, c->ps, h->device, h->ncols);
  int rc;
  if ((rc = fold_check(h, c))) return rc;
  HIPCHK(hipSetDevice(h->device));
  const long long N = c->chain_rows;
  if (N > 0 && (rc = reserve(h, c->W))) return rc;
  // [W][nrec][PS]: a walker's rows of this launch are one series
  return fold_run(h, c, N > 0 && c->W > 0, [&](hipStream_t s) {
    return launch_fold(h, s, c->d_chain, N * c->ps, c->ps, c->W, N);
  });
}

int olpe_acf_fold_rows(olpe_acf *h, const double *rows, long long nwalkers, long long nrows,
                       int time_major) {
  if (!h || nwalkers < 0 || nrows < 0 || (nwalkers > 0 && nrows > 0 && !rows))
    return set_err(OLPE_EINVAL, "bad argument");
  if (nwalkers == 0 || nrows == 0) return OLPE_OK;
  const size_t C = (size_t)h->ncols;
  const size_t ser_bytes = (size_t)nrows * C * 8;
  if (ser_bytes > kStageBytes)
    return set_err(OLPE_EINVAL, "a series of %lld rows x %d columns is %zu bytes; a piece of the "
                   "upload holds whole series and at most %zu bytes", nrows, h->ncols, ser_bytes,
                   (size_t)kStageBytes);
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  const long long per = std::min<long long>(nwalkers, (long long)(kStageBytes / ser_bytes));
  if ((rc = grow((void **)&h->d_stage, &h->stage_cap, (size_t)per * ser_bytes, "the row upload")))
    return rc;
  if ((rc = reserve(h, per))) return rc;
  for (long long w0 = 0; w0 < nwalkers; w0 += per) {
    const long long nw = std::min(per, nwalkers - w0);
    long long ws, rs;
    if (time_major) {
      // [N][W][C] -> [N][nw][C] on the device: a strided copy, no transposition
      HIPCHK(hipMemcpy2DAsync(h->d_stage, (size_t)nw * C * 8, rows + (size_t)w0 * C,
                              (size_t)nwalkers * C * 8, (size_t)nw * C * 8, (size_t)nrows,
                              hipMemcpyHostToDevice, h->stream));
      ws = (long long)C;
      rs = nw * (long long)C;
    } else {
      HIPCHK(hipMemcpyAsync(h->d_stage, rows + (size_t)w0 * nrows * C, (size_t)nw * ser_bytes,
                            hipMemcpyHostToDevice, h->stream));
      ws = nrows * (long long)C;
      rs = (long long)C;
    }
    if ((rc = launch_fold(h, h->stream, h->d_stage, ws, rs, nw, nrows))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));   // d_stage is reused
  }
  return OLPE_OK;
}

int olpe_acf_get(olpe_acf *h, unsigned long long *n, unsigned long long *series,
                 unsigned long long *skipped, double *C_out) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  unsigned long long cnt[3];
  HIPCHK(hipMemcpy(cnt, h->d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
  if (n) *n = cnt[0];
  if (series) *series = cnt[1];
  if (skipped) *skipped = cnt[2];
  if (C_out)
    HIPCHK(hipMemcpy(C_out, h->d_C, (size_t)h->ncols * (h->L + 1) * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

int olpe_acf_add(olpe_acf *h, int ncols, int max_lag, unsigned long long n,
                 unsigned long long series, unsigned long long skipped, const double *C_in) {
  if (!h || !C_in) return set_err(OLPE_EINVAL, "NULL argument");
  if (ncols != h->ncols || max_lag != h->L)
    return set_err(OLPE_EINVAL, "a state of %d columns and max_lag %d cannot be added to one of "
                   "%d columns and max_lag %d", ncols, max_lag, h->ncols, h->L);
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  // on the host: the state is a few hundred KB at the most
  const size_t nC = (size_t)h->ncols * (h->L + 1);
  std::vector<double> cur(nC);
  unsigned long long cnt[3];
  HIPCHK(hipMemcpy(cur.data(), h->d_C, nC * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cnt, h->d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < nC; ++i) cur[i] += C_in[i];
  cnt[0] += n;
  cnt[1] += series;
  cnt[2] += skipped;
  HIPCHK(hipMemcpy(h->d_C, cur.data(), nC * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
  return OLPE_OK;
}

int olpe_acf_reset(olpe_acf *h) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  HIPCHK(hipMemset(h->d_C, 0, (size_t)h->ncols * (h->L + 1) * 8));
  HIPCHK(hipMemset(h->d_cnt, 0, 3 * 8));
  fold_forget(h);
  return OLPE_OK;
}

}  // extern "C"
