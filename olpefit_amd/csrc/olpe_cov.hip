// olpe_cov.hip -- the cross-column sums of the recorded chains: what a parameter covariance,
// a correlation, an error ellipse, the conditional widths and the multivariate
// Gelman-Rubin statistic are functions of (olpefit_amd/covariance.py; the reference's
// corner figure, apf_step3.py:603-643, shows the pair scatter and gives no number for it).
// An olpe_cov keeps, about a fixed pivot p and with d = x - p per row,
//     n, skipped           rows folded, rows left out
//     S1[j]    = sum d_j
//     S2[j][k] = sum d_j d_k          (full matrix, the triangles bit-equal)
// and, created with walkers > 0, per walker w its row count nw[w] and S1w[w][j].  A row
// with a non-finite value in any column is left out whole and counted once.  The state is
// additive over folds, objects, ranks and checkpoints whose pivots are bit-equal.
//
// What the pivot costs: the sums hold (x - p), so a variance read from them as
// (S2 - S1^2 / n) / (n - 1) cancels (mean - p)^2 against sigma^2; its relative rounding
// error grows as 1 + (mean - p)^2 / sigma^2.  A pivot within a sigma of the mean (any row of
// a converged chain; step 3's column means) costs a factor of two at the most.
//
// Kernels, the vector form:
//   * cov_pivot_kernel: with no pivot yet, the first row folded becomes it (a non-finite
//     entry 0.0).
//   * cov_fold_kernel<CP, TR>, CP = the columns rounded up to a multiple of 4.  A tile is
//     TR = 256 consecutive rows of one walker (64 or 128 with OLPE_COV_TILE, a test knob).  A workgroup of 8 waves owns a fixed run of tiles;
//     per tile it stages d in LDS (row pitch CP + 1 doubles: odd, so lane = row reads are
//     conflict-free), zeroes the rows that hold a non-finite value, and then every wave
//     walks the rows, lane = row, over its share of the 4 x 4 column blocks of the upper
//     triangle (at most 3 blocks = 48 accumulators a lane), which stay in registers over
//     all of the workgroup's tiles.  The next tile's loads are in flight meanwhile.  Each
//     wave also sums the columns of an eighth of the tile's rows, lane = column, in row order,
//     and the last wave adds the eight in wave order: the tile's S1, which is stored per
//     tile when the object keeps walkers.  The cross-lane reduction (a
//     fixed butterfly) happens once per workgroup.
//   * cov_reduce_kernel adds the workgroups' partial sums in a fixed tree, cov_walker_kernel
//     a walker's tiles in tile order.  cov_between_kernel: the between-walker term.
// No floating-point atomics: the runs of tiles are a function of the fold's shape alone,
// so the same fold of the same rows gives the same bits on any device or grid.
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

struct olpe_cov : FoldBase {
  int ncols = 0, CP = 0;
  int tile = 0;                         // rows of a tile (OLPE_COV_TILE, else the default)
  long long walkers = 0;
  bool pivot_given = false, has_pivot = false;
  double *d_pivot = nullptr;            // [ncols]
  double *d_S1 = nullptr;               // [ncols]
  double *d_S2 = nullptr;               // [ncols][ncols]
  unsigned long long *d_cnt = nullptr;  // {n, skipped}
  double *d_S1w = nullptr;              // [walkers][ncols]
  unsigned long long *d_nw = nullptr;   // [walkers]
  double *d_part = nullptr;             // [kMaxSlots][CP * CP + CP] workgroup partials
  unsigned long long *d_partn = nullptr;  // [kMaxSlots] rows kept
  double *d_between = nullptr;          // [ncols][ncols], then 3 words {m, min nw, max nw}
  // per-fold work buffers, grown on demand
  double *d_tile_s1 = nullptr;          // [tiles][ncols]
  unsigned *d_tile_n = nullptr;         // [tiles]
  size_t tile_cap = 0;
  double *d_stage = nullptr;            // upload staging of fold_rows
  size_t stage_cap = 0;
};

namespace {

constexpr int kMaxCols = 24;
constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kTiles[] = {64, 128, 256};          // rows of a tile (OLPE_COV_TILE)
constexpr int kDefaultTile = 256;
constexpr int kMaxSlots = 2048;                   // workgroups (partial sums) of a fold
constexpr int kRedThreads = 256;
constexpr long long kMaxWalkers = 65535ll * 64;   // as olpe_phot's
constexpr size_t kStageBytes = 256ull << 20;      // fold_rows uploads pieces of this size

struct FoldArgs {
  const double *x;            // value (walker w, row t, column c) at x[w * ws + t * rs + c]
  long long ws, rs;
  long long N;                // rows per walker
  int C;
  long long tpw;              // tiles per walker
  long long tiles, chunk;     // walkers x tpw, tiles per workgroup
  const double *pivot;
  double *part;
  unsigned long long *partn;
  double *tile_s1;            // null: the tiles' sums are not kept
  unsigned *tile_n;
};

__global__ void cov_pivot_kernel(const double *__restrict__ x, int C, double *__restrict__ pivot) {
  const int c = threadIdx.x;
  if (c < C) {
    const double v = x[c];
    pivot[c] = isfinite(v) ? v : 0.0;
  }
}

// Up to 12 columns two workgroups share a CU: 4 waves a SIMD, 128 VGPRs.  Above, one
// workgroup has the CU and up to 256 VGPRs: the 32 or 48 accumulators a lane, and the next
// tile's 16 values a thread in flight.
template <int CP, int TR>
__global__ __launch_bounds__(kThreads, CP <= 12 ? 4 : 2) void
cov_fold_kernel(const FoldArgs a) {
  constexpr int G = CP / 4, NB = G * (G + 1) / 2, NBW = (NB + kWaves - 1) / kWaves;
  // staging lanes per row: a power of two that holds the columns (and a trip the tile)
  constexpr int LW0 = CP <= 4 ? 4 : CP <= 8 ? 8 : CP <= 16 ? 16 : 32;
  constexpr int LW = LW0 * TR < kThreads ? kThreads / TR : LW0;
  constexpr int RG = kThreads / LW;               // rows staged per trip
  constexpr int K = TR / RG;               // trips per tile
  constexpr int PITCH = CP + 1;
  __shared__ double sx[TR * PITCH];
  __shared__ int sbad[2][TR];
  __shared__ double spart[2][kWaves][32];          // the waves' column sums of a tile
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.C;
  // the wave's column blocks (gi <= gj), block id wave + b * kWaves in row-major order
  int ci[NBW], cj[NBW];
  bool on[NBW];
#pragma unroll
  for (int b = 0; b < NBW; ++b) {
    int rem = wave + b * kWaves, gi = 0;
    on[b] = rem < NB;
    if (!on[b]) rem = 0;
    while (rem >= G - gi) {
      rem -= G - gi;
      ++gi;
    }
    ci[b] = gi * 4;
    cj[b] = (gi + rem) * 4;
  }
  double acc[NBW][4][4];
#pragma unroll
  for (int b = 0; b < NBW; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[b][i][j] = 0.0;
  double s1_block = 0.0;                           // last wave, lane = column
  unsigned long long n_block = 0;
  for (int i = tid; i < TR * PITCH; i += kThreads) sx[i] = 0.0;  // the pad columns stay 0
  if (tid < TR) sbad[0][tid] = sbad[1][tid] = 0;
  const int sc = tid % LW, sr = tid / LW;          // staging: column, first row
  const bool scol = sc < C;
  const double pc = scol ? a.pivot[sc] : 0.0;
  const long long q0 = (long long)blockIdx.x * a.chunk;
  const long long q1 = q0 + a.chunk < a.tiles ? q0 + a.chunk : a.tiles;
  double v[K];
  // the loads of tile q (a row past the walker's last, or a lane past the columns, reads nothing)
  auto load = [&](long long q) {
    const long long w = q / a.tpw, t0 = (q - w * a.tpw) * TR;
    const double *base = a.x + (size_t)w * a.ws + (size_t)t0 * a.rs + sc;
    const long long left = a.N - t0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int r = sr + k * RG;
      v[k] = scol && r < left ? base[(size_t)r * a.rs] : pc;
    }
  };
  // the last wave, a tile later: the waves' column sums of tile qq in wave order
  auto finish = [&](long long qq, int pp, unsigned kept) {
    double s = 0.0;
#pragma unroll
    for (int v8 = 0; v8 < kWaves; ++v8) s += spart[pp][v8][lane & 31];
    s1_block += s;
    n_block += kept;
    if (a.tile_s1) {
      if (lane < C) a.tile_s1[(size_t)qq * C + lane] = s;
      if (lane == 0) a.tile_n[qq] = kept;
    }
  };
  if (q0 < q1) load(q0);
  int par = 0;
  unsigned kept_prev = 0;
  for (long long q = q0; q < q1; ++q, par ^= 1) {
    const long long w = q / a.tpw, t0 = (q - w * a.tpw) * TR;
    const int nrows = (int)(a.N - t0 < TR ? a.N - t0 : TR);
    __syncthreads();                               // the last tile's walks are done
    if (scol) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int r = sr + k * RG;
        if (!isfinite(v[k])) sbad[par][r] = 1;     // every writer stores the same 1
        sx[r * PITCH + sc] = v[k] - pc;            // exactly 0.0 past the last row
      }
    }
    __syncthreads();
    if (tid < TR) {
      if (sbad[par][tid])
        for (int c = 0; c < C; ++c) sx[tid * PITCH + c] = 0.0;
      sbad[par ^ 1][tid] = 0;                      // the next tile's flags
    }
    __syncthreads();
    if (q + 1 < q1) load(q + 1);                   // in flight during the walks
    if (wave == kWaves - 1 && q > q0) finish(q - 1, par ^ 1, kept_prev);
#pragma unroll
    for (int h = 0; h < TR / 64; ++h) {
      const double *xr = sx + (lane + 64 * h) * PITCH;
#pragma unroll
      for (int b = 0; b < NBW; ++b) {
        if (!on[b]) continue;                      // the same for the whole wave
        double xi[4], xj[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xi[i] = xr[ci[b] + i];
          xj[i] = xr[cj[b] + i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[b][i][j] = __builtin_fma(xi[i], xj[j], acc[b][i][j]);
      }
    }
    {
      // the column sums of the wave's TR / 8 rows, lane = column, in row order: lanes 0 .. 31
      // the first half of them, lanes 32 .. 63 the second (the rows left out and the rows
      // past the last hold 0.0), then the two halves; the last wave adds the waves' sums
      // while the next tile is walked
      const int c = (lane & 31) < CP ? (lane & 31) : 0;
      const double *xc = sx + (wave * (TR / 8) + (lane >> 5) * (TR / 16)) * PITCH + c;
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < TR / 16; ++r) s += xc[r * PITCH];
      s += __shfl(s, (lane + 32) & 63, 64);
      if (lane < 32) spart[par][wave][lane] = s;
    }
    if (wave == kWaves - 1) {
      kept_prev = (unsigned)nrows;
#pragma unroll
      for (int h = 0; h < TR / 64; ++h)
        kept_prev -= (unsigned)__popcll(__ballot(sbad[par][lane + 64 * h] != 0));
    }
  }
  __syncthreads();
  if (wave == kWaves - 1 && q0 < q1) finish(q1 - 1, par ^ 1, kept_prev);
  // the lanes' sums by a fixed butterfly: every lane ends with the same bits
#pragma unroll
  for (int b = 0; b < NBW; ++b)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double s = acc[b][i][j];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
        acc[b][i][j] = s;
      }
  double *out = a.part + (size_t)blockIdx.x * (CP * CP + CP);
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < NBW; ++b)
      if (on[b])
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) out[(ci[b] + i) * CP + cj[b] + j] = acc[b][i][j];
  }
  if (wave == kWaves - 1) {
    if (lane < CP) out[CP * CP + lane] = s1_block;
    if (lane == 0) a.partn[blockIdx.x] = n_block;
  }
}

// A workgroup per output: S2[j][k] for j <= k (blocks 0 .. C C - 1; j > k has nothing to
// do), S1[c] (C C .. C C + C - 1), the counters (the last).  Thread i adds the partial sums
// of workgroups i, i + 256, ..., then the fixed tree.
__global__ __launch_bounds__(kRedThreads) void cov_reduce_kernel(
    const double *__restrict__ part, const unsigned long long *__restrict__ partn, int slots,
    int C, int CP, unsigned long long rows, double *__restrict__ S1, double *__restrict__ S2,
    unsigned long long *__restrict__ cnt) {
  __shared__ double red[kRedThreads];
  __shared__ unsigned long long redn[kRedThreads];
  const int o = blockIdx.x;
  const size_t stride = (size_t)CP * CP + CP;
  if (o < C * C + C) {
    int at;
    const int j = o / C, k = o - j * C;
    if (o < C * C) {
      if (j > k) return;
      at = j * CP + k;
    } else {
      at = CP * CP + (o - C * C);
    }
    double s = 0.0;
    for (int b = threadIdx.x; b < slots; b += kRedThreads) s += part[(size_t)b * stride + at];
    const double tot = block_sum<kRedThreads>(s, red);
    if (threadIdx.x == 0) {
      if (o < C * C) {
        const double nv = S2[j * C + k] + tot;
        S2[j * C + k] = nv;
        S2[k * C + j] = nv;
      } else {
        S1[o - C * C] += tot;
      }
    }
    return;
  }
  unsigned long long n = 0;
  for (int b = threadIdx.x; b < slots; b += kRedThreads) n += partn[b];
  n = block_word<kRedThreads, WordSum>(n, redn);
  if (threadIdx.x == 0) {
    cnt[0] += n;
    cnt[1] += rows - n;
  }
}

// thread (w, c): walker w0 + w's tiles in tile order; c == C is the row count
__global__ __launch_bounds__(kRedThreads) void cov_walker_kernel(
    const double *__restrict__ tile_s1, const unsigned *__restrict__ tile_n, long long W,
    long long tpw, int C, long long w0, double *__restrict__ S1w,
    unsigned long long *__restrict__ nw) {
  const long long i = (long long)blockIdx.x * kRedThreads + threadIdx.x;
  if (i >= W * (C + 1)) return;
  const long long w = i / (C + 1);
  const int c = (int)(i - w * (C + 1));
  if (c < C) {
    double s = 0.0;
    for (long long t = 0; t < tpw; ++t) s += tile_s1[(size_t)(w * tpw + t) * C + c];
    S1w[(size_t)(w0 + w) * C + c] += s;
  } else {
    unsigned long long n = 0;
    for (long long t = 0; t < tpw; ++t) n += tile_n[w * tpw + t];
    nw[w0 + w] += n;
  }
}

// A workgroup per pair j <= k: sum over the walkers with rows of S1w[w][j] S1w[w][k] / nw[w]
// (thread i walkers i, i + 256, ..., then the fixed tree) into both triangles; workgroup 0
// also counts those walkers and takes the extremes of nw.
__global__ __launch_bounds__(kRedThreads) void cov_between_kernel(
    const double *__restrict__ S1w, const unsigned long long *__restrict__ nw, long long W, int C,
    double *__restrict__ out) {
  __shared__ double red[kRedThreads];
  __shared__ unsigned long long rw[kRedThreads];
  const int j = blockIdx.x / C, k = blockIdx.x - j * C;
  if (j > k) return;
  double s = 0.0;
  unsigned long long m = 0, lo = ~0ull, hi = 0;
  for (long long w = threadIdx.x; w < W; w += kRedThreads) {
    const unsigned long long n = nw[w];
    if (!n) continue;
    s += (S1w[(size_t)w * C + j] * S1w[(size_t)w * C + k]) / (double)n;
    ++m;
    lo = n < lo ? n : lo;
    hi = n > hi ? n : hi;
  }
  const double tot = block_sum<kRedThreads>(s, red);
  if (threadIdx.x == 0) {
    out[j * C + k] = tot;
    out[k * C + j] = tot;
  }
  if (blockIdx.x) return;
  m = block_word<kRedThreads, WordSum>(m, rw);
  lo = block_word<kRedThreads, WordMin>(lo, rw);
  hi = block_word<kRedThreads, WordMax>(hi, rw);
  if (threadIdx.x == 0) {
    unsigned long long *ow = reinterpret_cast<unsigned long long *>(out + (size_t)C * C);
    ow[0] = m;
    ow[1] = m ? lo : 0;
    ow[2] = hi;
  }
}

size_t part_stride(const olpe_cov *h) { return (size_t)h->CP * h->CP + h->CP; }

// the tiles' sums of a fold of `tiles` tiles (drained first: the buffers may be replaced)
int reserve(olpe_cov *h, long long tiles) {
  if (!h->walkers || (size_t)tiles <= h->tile_cap) return OLPE_OK;
  int rc;
  if ((rc = drain(h))) return rc;
  if (h->d_tile_s1) (void)hipFree(h->d_tile_s1);
  if (h->d_tile_n) (void)hipFree(h->d_tile_n);
  h->d_tile_s1 = nullptr;
  h->d_tile_n = nullptr;
  h->tile_cap = 0;
  if ((rc = alloc((void **)&h->d_tile_s1, (size_t)tiles * h->ncols * 8, "the tiles' column sums")))
    return rc;
  if ((rc = alloc((void **)&h->d_tile_n, (size_t)tiles * sizeof(unsigned), "the tiles' row counts")))
    return rc;
  h->tile_cap = (size_t)tiles;
  return OLPE_OK;
}

long long tiles_of(const olpe_cov *h, long long W, long long N) {
  return W * ((N + h->tile - 1) / h->tile);
}

// the kernels over W walkers of N rows at d_x, on `stream`; w0 = the first one's index
int launch_fold(olpe_cov *h, hipStream_t stream, const double *d_x, long long ws, long long rs,
                long long W, long long N, long long w0) {
  const int C = h->ncols;
  if (!h->has_pivot) {
    hipLaunchKernelGGL(cov_pivot_kernel, dim3(1), dim3(64), 0, stream, d_x, C, h->d_pivot);
    HIPCHK(hipGetLastError());
  }
  FoldArgs a = {};
  a.x = d_x;
  a.ws = ws;
  a.rs = rs;
  a.N = N;
  a.C = C;
  a.tpw = (N + h->tile - 1) / h->tile;
  a.tiles = W * a.tpw;
  long long slots = std::min<long long>(a.tiles, kMaxSlots);
  a.chunk = (a.tiles + slots - 1) / slots;
  slots = (a.tiles + a.chunk - 1) / a.chunk;
  a.pivot = h->d_pivot;
  a.part = h->d_part;
  a.partn = h->d_partn;
  a.tile_s1 = h->walkers ? h->d_tile_s1 : nullptr;
  a.tile_n = h->walkers ? h->d_tile_n : nullptr;
  const dim3 grid((unsigned)slots), block(kThreads);
#define OLPE_COV_LAUNCH(CP_)                                                              \
  case CP_:                                                                              \
    if (h->tile == 64)                                                                   \
      hipLaunchKernelGGL((cov_fold_kernel<CP_, 64>), grid, block, 0, stream, a);         \
    else if (h->tile == 128)                                                             \
      hipLaunchKernelGGL((cov_fold_kernel<CP_, 128>), grid, block, 0, stream, a);        \
    else                                                                                 \
      hipLaunchKernelGGL((cov_fold_kernel<CP_, 256>), grid, block, 0, stream, a);        \
    break;
  switch (h->CP) {
    OLPE_COV_LAUNCH(4)
    OLPE_COV_LAUNCH(8)
    OLPE_COV_LAUNCH(12)
    OLPE_COV_LAUNCH(16)
    OLPE_COV_LAUNCH(20)
    OLPE_COV_LAUNCH(24)
  }
#undef OLPE_COV_LAUNCH
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(cov_reduce_kernel, dim3(C * C + C + 1), dim3(kRedThreads), 0, stream,
                     h->d_part, h->d_partn, (int)slots, C, h->CP, (unsigned long long)(W * N),
                     h->d_S1, h->d_S2, h->d_cnt);
  HIPCHK(hipGetLastError());
  if (h->walkers) {
    const long long nthr = W * (C + 1);
    hipLaunchKernelGGL(cov_walker_kernel, dim3((unsigned)((nthr + kRedThreads - 1) / kRedThreads)),
                       dim3(kRedThreads), 0, stream, h->d_tile_s1, h->d_tile_n, W, a.tpw, C, w0,
                       h->d_S1w, h->d_nw);
    HIPCHK(hipGetLastError());
  }
  h->has_pivot = true;                             // the first row's, once every launch is queued
  return OLPE_OK;
}

int zero_state(olpe_cov *h) {
  const size_t C = (size_t)h->ncols;
  HIPCHK(hipMemset(h->d_S1, 0, C * 8));
  HIPCHK(hipMemset(h->d_S2, 0, C * C * 8));
  HIPCHK(hipMemset(h->d_cnt, 0, 2 * 8));
  if (h->walkers) {
    HIPCHK(hipMemset(h->d_S1w, 0, (size_t)h->walkers * C * 8));
    HIPCHK(hipMemset(h->d_nw, 0, (size_t)h->walkers * 8));
  }
  return OLPE_OK;
}

}  // namespace

extern "C" {

int olpe_cov_create(int device, int ncols, long long walkers, const double *pivot,
                    olpe_cov **out) {
  if (!out) return set_err(OLPE_EINVAL, "NULL out");
  *out = nullptr;
  if (ncols < 1 || ncols > kMaxCols)
    return set_err(OLPE_EINVAL, "ncols %d: 1 to %d columns", ncols, kMaxCols);
  if (walkers < 0 || walkers > kMaxWalkers)
    return set_err(OLPE_EINVAL, "walkers %lld: 0 (pooled only) to %lld", walkers, kMaxWalkers);
  if (pivot)
    for (int c = 0; c < ncols; ++c)
      if (!isfinite(pivot[c])) return set_err(OLPE_EINVAL, "non-finite pivot of column %d", c);
  int tile = kDefaultTile;
  if (const char *t = getenv("OLPE_COV_TILE")) {
    char *end = nullptr;
    const long v = strtol(t, &end, 10);
    if (!*t || *end || std::find(std::begin(kTiles), std::end(kTiles), v) == std::end(kTiles))
      return set_err(OLPE_EINVAL, "OLPE_COV_TILE=%s: 64, 128 or 256", t);
    tile = (int)v;
  }
  int rc;
  if ((rc = open_device(device))) return rc;
  olpe_cov *h = new olpe_cov;
  h->ncols = ncols;
  h->tile = tile;
  h->CP = (ncols + 3) / 4 * 4;
  h->walkers = walkers;
  h->pivot_given = h->has_pivot = pivot != nullptr;
  const size_t C = (size_t)ncols;
  rc = fold_open(h, device);
  if (!rc) rc = alloc((void **)&h->d_pivot, C * 8, "the pivot");
  if (!rc) rc = alloc((void **)&h->d_S1, C * 8, "the column sums");
  if (!rc) rc = alloc((void **)&h->d_S2, C * C * 8, "the cross-product sums");
  if (!rc) rc = alloc((void **)&h->d_cnt, 2 * 8, "the counters");
  if (!rc) rc = alloc((void **)&h->d_between, (C * C + 3) * 8, "the between-walker term");
  if (!rc) rc = alloc((void **)&h->d_part, kMaxSlots * part_stride(h) * 8, "the partial sums");
  if (!rc) rc = alloc((void **)&h->d_partn, kMaxSlots * 8, "the partial counts");
  if (!rc && walkers) rc = alloc((void **)&h->d_S1w, (size_t)walkers * C * 8, "the walkers' sums");
  if (!rc && walkers) rc = alloc((void **)&h->d_nw, (size_t)walkers * 8, "the walkers' counts");
  if (!rc) rc = zero_state(h);
  if (!rc && hipMemset(h->d_pivot, 0, C * 8) != hipSuccess) rc = set_err(OLPE_EHIP, "hipMemset failed");
  if (!rc && pivot && hipMemcpy(h->d_pivot, pivot, C * 8, hipMemcpyHostToDevice) != hipSuccess)
    rc = set_err(OLPE_EHIP, "the pivot's upload failed");
  if (rc) {
    olpe_cov_destroy(h);
    return rc;
  }
  *out = h;
  return OLPE_OK;
}

void olpe_cov_destroy(olpe_cov *h) {
  if (!h) return;
  fold_close(h, {h->d_pivot, h->d_S1, h->d_S2, h->d_cnt, h->d_S1w, h->d_nw, h->d_part,
                 h->d_partn, h->d_between, h->d_tile_s1, h->d_tile_n, h->d_stage});
  delete h;
}

int olpe_cov_fold_ctx(olpe_cov *h, olpe_ctx *c, int row_step) {
  if (!h || !c) return set_err(OLPE_EINVAL, "NULL argument");
  if (row_step < 1) return set_err(OLPE_EINVAL, "row_step %d: must be >= 1", row_step);
  if (c->device != h->device || c->ps != h->ncols)
    return set_err(OLPE_EINVAL, "context of device %d, PS %d; covariance of device %d, %d columns",
                   c->device, c->ps, h->device, h->ncols);
  if (h->walkers && h->walkers != c->W)
    return set_err(OLPE_EINVAL, "context of %d walkers; covariance of %lld walkers", c->W,
                   h->walkers);
  int rc;
  if ((rc = fold_check(h, c))) return rc;
  HIPCHK(hipSetDevice(h->device));
  // rows 0, row_step, ... of the chain [W][nrec][PS]: indexing only
  const long long N = (c->chain_rows + row_step - 1) / row_step;
  if (N > 0 && c->W > 0 && (rc = reserve(h, tiles_of(h, c->W, N)))) return rc;
  return fold_run(h, c, N > 0 && c->W > 0, [&](hipStream_t s) {
    return launch_fold(h, s, c->d_chain, c->chain_rows * c->ps, (long long)row_step * c->ps,
                       c->W, N, 0);
  });
}

int olpe_cov_fold_rows(olpe_cov *h, const double *rows, long long nwalkers, long long nrows,
                       int time_major) {
  if (!h || nwalkers < 0 || nrows < 0 || (nwalkers > 0 && nrows > 0 && !rows))
    return set_err(OLPE_EINVAL, "bad argument");
  if (h->walkers && nwalkers != h->walkers)
    return set_err(OLPE_EINVAL, "rows of %lld walkers; covariance of %lld walkers", nwalkers,
                   h->walkers);
  if (nwalkers == 0 || nrows == 0) return OLPE_OK;
  const size_t C = (size_t)h->ncols;
  if (!h->walkers) {                               // pooled only: the two dimensions are rows
    if (nwalkers > (1ll << 40) / nrows) return set_err(OLPE_EINVAL, "%lld x %lld rows", nwalkers, nrows);
    nrows *= nwalkers;
    nwalkers = 1;
    time_major = 0;
  }
  const size_t row_bytes = C * 8;
  if (time_major && (size_t)nwalkers * row_bytes > kStageBytes)
    return set_err(OLPE_EINVAL, "one row of %lld walkers x %d columns is %zu bytes; a piece of "
                   "the upload holds whole rows and at most %zu bytes", nwalkers, h->ncols,
                   (size_t)nwalkers * row_bytes, (size_t)kStageBytes);
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  // pieces as the rows lie: time-major runs of rows of every walker, else runs of whole
  // walkers, or of one walker's rows where a walker exceeds a piece
  long long pw, pr;                                // walkers, rows per piece
  if (time_major) {
    pw = nwalkers;
    pr = std::min<long long>(nrows, std::max<long long>(1, (long long)(kStageBytes / (pw * row_bytes))));
  } else if ((size_t)nrows * row_bytes <= kStageBytes) {
    pr = nrows;
    pw = std::min<long long>(nwalkers, (long long)(kStageBytes / ((size_t)nrows * row_bytes)));
  } else {
    pw = 1;
    pr = (long long)(kStageBytes / row_bytes);
  }
  if ((rc = grow((void **)&h->d_stage, &h->stage_cap, (size_t)pw * pr * row_bytes, "the row upload")))
    return rc;
  if ((rc = reserve(h, tiles_of(h, pw, pr)))) return rc;
  for (long long w0 = 0; w0 < nwalkers; w0 += pw)
    for (long long r0 = 0; r0 < nrows; r0 += pr) {
      const long long nw = std::min(pw, nwalkers - w0), nr = std::min(pr, nrows - r0);
      long long ws, rs;
      const double *src;
      if (time_major) {
        src = rows + (size_t)r0 * nwalkers * C;
        ws = (long long)C;
        rs = nwalkers * (long long)C;
      } else {
        src = rows + ((size_t)w0 * nrows + r0) * C;
        ws = nr * (long long)C;
        rs = (long long)C;
      }
      HIPCHK(hipMemcpyAsync(h->d_stage, src, (size_t)nw * nr * row_bytes, hipMemcpyHostToDevice,
                            h->stream));
      if ((rc = launch_fold(h, h->stream, h->d_stage, ws, rs, nw, nr, w0))) return rc;
      HIPCHK(hipStreamSynchronize(h->stream));     // d_stage is reused
    }
  return OLPE_OK;
}

int olpe_cov_get(olpe_cov *h, unsigned long long *n, unsigned long long *skipped,
                 int *has_pivot, double *pivot, double *S1, double *S2) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  const size_t C = (size_t)h->ncols;
  unsigned long long cnt[2];
  HIPCHK(hipMemcpy(cnt, h->d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
  if (n) *n = cnt[0];
  if (skipped) *skipped = cnt[1];
  if (has_pivot) *has_pivot = h->has_pivot ? 1 : 0;
  if (pivot) HIPCHK(hipMemcpy(pivot, h->d_pivot, C * 8, hipMemcpyDeviceToHost));
  if (S1) HIPCHK(hipMemcpy(S1, h->d_S1, C * 8, hipMemcpyDeviceToHost));
  if (S2) HIPCHK(hipMemcpy(S2, h->d_S2, C * C * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

int olpe_cov_walkers_get(olpe_cov *h, unsigned long long *nw, double *S1w) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  if (!h->walkers) return set_err(OLPE_ESTATE, "created with walkers 0: pooled sums only");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  if (nw) HIPCHK(hipMemcpy(nw, h->d_nw, (size_t)h->walkers * 8, hipMemcpyDeviceToHost));
  if (S1w)
    HIPCHK(hipMemcpy(S1w, h->d_S1w, (size_t)h->walkers * h->ncols * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

int olpe_cov_between(olpe_cov *h, double *B, unsigned long long *m, unsigned long long *nw_min,
                     unsigned long long *nw_max) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  if (!h->walkers) return set_err(OLPE_ESTATE, "created with walkers 0: pooled sums only");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  const int C = h->ncols;
  hipLaunchKernelGGL(cov_between_kernel, dim3(C * C), dim3(kRedThreads), 0, h->stream, h->d_S1w,
                     h->d_nw, h->walkers, C, h->d_between);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  unsigned long long w[3];
  HIPCHK(hipMemcpy(w, h->d_between + (size_t)C * C, sizeof w, hipMemcpyDeviceToHost));
  if (B) HIPCHK(hipMemcpy(B, h->d_between, (size_t)C * C * 8, hipMemcpyDeviceToHost));
  if (m) *m = w[0];
  if (nw_min) *nw_min = w[1];
  if (nw_max) *nw_max = w[2];
  return OLPE_OK;
}

int olpe_cov_add(olpe_cov *h, int ncols, long long walkers, unsigned long long n,
                 unsigned long long skipped, const double *pivot, const double *S1,
                 const double *S2, const unsigned long long *nw, const double *S1w) {
  if (!h || !pivot || !S1 || !S2) return set_err(OLPE_EINVAL, "NULL argument");
  if (ncols != h->ncols)
    return set_err(OLPE_EINVAL, "a state of ncols %d cannot be added to one of ncols %d", ncols,
                   h->ncols);
  if (walkers != h->walkers)
    return set_err(OLPE_EINVAL, "a state of walkers %lld cannot be added to one of walkers %lld",
                   walkers, h->walkers);
  if (walkers && (!nw || !S1w)) return set_err(OLPE_EINVAL, "NULL walker sums");
  const size_t C = (size_t)ncols;
  for (size_t c = 0; c < C; ++c)
    if (!isfinite(pivot[c])) return set_err(OLPE_EINVAL, "non-finite pivot of column %zu", c);
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  if (h->has_pivot) {
    std::vector<double> p(C);
    HIPCHK(hipMemcpy(p.data(), h->d_pivot, C * 8, hipMemcpyDeviceToHost));
    for (size_t c = 0; c < C; ++c)
      if (memcmp(&p[c], &pivot[c], 8))
        return set_err(OLPE_EINVAL, "the pivot differs in column %zu (%.17g here, %.17g "
                       "incoming): rebase one state first", c, p[c], pivot[c]);
  }
  // on the host: the pooled state is a few KB, the walkers' 8 (ncols + 1) bytes each
  std::vector<double> s1(C), s2(C * C);
  unsigned long long cnt[2];
  HIPCHK(hipMemcpy(s1.data(), h->d_S1, C * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(s2.data(), h->d_S2, C * C * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(cnt, h->d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < C; ++i) s1[i] += S1[i];
  for (size_t j = 0; j < C; ++j)
    for (size_t k = j; k < C; ++k) {
      s2[j * C + k] += S2[j * C + k];
      s2[k * C + j] = s2[j * C + k];
    }
  cnt[0] += n;
  cnt[1] += skipped;
  if (walkers) {
    const size_t W = (size_t)walkers;
    std::vector<double> sw(W * C);
    std::vector<unsigned long long> cw(W);
    HIPCHK(hipMemcpy(sw.data(), h->d_S1w, W * C * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cw.data(), h->d_nw, W * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < W * C; ++i) sw[i] += S1w[i];
    for (size_t i = 0; i < W; ++i) cw[i] += nw[i];
    HIPCHK(hipMemcpy(h->d_S1w, sw.data(), W * C * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_nw, cw.data(), W * 8, hipMemcpyHostToDevice));
  }
  HIPCHK(hipMemcpy(h->d_S1, s1.data(), C * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_S2, s2.data(), C * C * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_cnt, cnt, sizeof cnt, hipMemcpyHostToDevice));
  if (!h->has_pivot) {
    HIPCHK(hipMemcpy(h->d_pivot, pivot, C * 8, hipMemcpyHostToDevice));
    h->has_pivot = true;
  }
  return OLPE_OK;
}

int olpe_cov_reset(olpe_cov *h) {
  if (!h) return set_err(OLPE_EINVAL, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if ((rc = drain(h))) return rc;
  if ((rc = zero_state(h))) return rc;
  if (!h->pivot_given) {
    HIPCHK(hipMemset(h->d_pivot, 0, (size_t)h->ncols * 8));
    h->has_pivot = false;
  }
  fold_forget(h);
  return OLPE_OK;
}

}  // extern "C"
