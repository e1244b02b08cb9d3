// olpe_samples.h -- the front end that the per-pixel folds over samples (olpe_resid.hip,
// olpe_lik.hip) share: how a piece of samples is scanned for usable rows, booked (compact
// offsets, counts, best row, pivot) and turned into model descriptors at compact positions,
// and sweep_exact's per-pixel expression on such a descriptor.  Device code and constants
// only; each unit includes it once, after it has included olpe_device.h in a namespace of
// its own and named that namespace's `olpe` as `dev`.  Everything here has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <limits.h>
#include <math.h>

#include <cmath>

namespace {

constexpr int kB = 256;                        // samples per block: the unit of summation order
constexpr int kThreads = 256;
constexpr int kMaxPieceBlocks = 1024;          // 64x64, 16-row tiles: 4096 waves, the chip once
constexpr size_t kPartBudget = 64u << 20;      // bytes of partials a piece aims at
constexpr size_t kPartLimit = 1u << 30;        // ... and may not exceed (one block of a huge frame)
// d_words
enum { kWUsed = 0, kWBad, kWHavePivot, kWPivotNew, kWHaveBest, kWPiece, kWords = 8 };

struct BlkInfo {
  int cnt, bad, first, best;    // usable rows, unusable rows, first usable row, best row
  double chi;                   // (INT_MAX: none); rows counted from the block's start
};

// sample s of a fold -> its row: s = w * rn + r at base + w * sw + r * sr
struct RowMap {
  const double *base;
  long long rn, sw, sr;
};
__device__ __forceinline__ const double *row_of(const RowMap &m, long long s) {
  const long long w = s / m.rn;
  return m.base + w * m.sw + (s - w * m.rn) * m.sr;
}

template <int NP> __device__ __forceinline__ bool usable_row(const double *row) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < NP; ++k) ok = ok && isfinite(row[k]);
  return ok;
}

// (chi2, i2) beats (chi1, i1): smaller chi^2, the earlier row on a tie; INT_MAX = none
__device__ __forceinline__ bool beats(double chi2, int i2, double chi1, int i1) {
  if (i2 == INT_MAX) return false;
  if (i1 == INT_MAX) return true;
  return chi2 < chi1 || (chi2 == chi1 && i2 < i1);
}

// 1. scan: block b = rows [b * kB, ...) of the piece's ns samples starting at sample s0
template <int NP>
__global__ __launch_bounds__(kThreads) void resid_scan_kernel(RowMap m, long long s0, int ns,
                                                              BlkInfo *__restrict__ info) {
  __shared__ int s_cnt[kThreads], s_bad[kThreads], s_first[kThreads], s_best[kThreads];
  __shared__ double s_chi[kThreads];
  const int t = threadIdx.x;
  const int s = blockIdx.x * kB + t;
  bool ok = false;
  double chi = 0.0;
  if (s < ns) {
    const double *row = row_of(m, s0 + s);
    ok = usable_row<NP>(row);
    chi = row[NP];
  }
  s_cnt[t] = ok;
  s_bad[t] = s < ns && !ok;
  s_first[t] = ok ? t : INT_MAX;
  s_best[t] = ok && chi == chi ? t : INT_MAX;
  s_chi[t] = chi;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
      s_cnt[t] += s_cnt[t + o];
      s_bad[t] += s_bad[t + o];
      s_first[t] = min(s_first[t], s_first[t + o]);
      if (beats(s_chi[t + o], s_best[t + o], s_chi[t], s_best[t])) {
        s_chi[t] = s_chi[t + o];
        s_best[t] = s_best[t + o];
      }
    }
    __syncthreads();
  }
  if (t == 0) info[blockIdx.x] = BlkInfo{s_cnt[0], s_bad[0], s_first[0], s_best[0], s_chi[0]};
}

// 2. book: one workgroup, a thread per block of the piece
template <int PS>
__global__ __launch_bounds__(kMaxPieceBlocks) void resid_book_kernel(
    RowMap m, long long s0, int nblk, const BlkInfo *__restrict__ info, int *__restrict__ boff,
    unsigned long long *__restrict__ words, double *__restrict__ pivot,
    double *__restrict__ best) {
  __shared__ int s_off[kMaxPieceBlocks], s_bad[kMaxPieceBlocks], s_first[kMaxPieceBlocks],
      s_best[kMaxPieceBlocks];
  __shared__ double s_chi[kMaxPieceBlocks];
  __shared__ int s_take[2];     // rows of the piece to copy: the best, the pivot (-1: none)
  const int t = threadIdx.x;
  const BlkInfo q = t < nblk ? info[t] : BlkInfo{0, 0, INT_MAX, INT_MAX, 0.0};
  s_off[t] = q.cnt;
  s_bad[t] = q.bad;
  s_first[t] = q.first == INT_MAX ? INT_MAX : t * kB + q.first;
  s_best[t] = q.best == INT_MAX ? INT_MAX : t * kB + q.best;
  s_chi[t] = q.chi;
  __syncthreads();
  for (int o = 1; o < kMaxPieceBlocks; o <<= 1) {      // inclusive scan of the counts
    const int v = t >= o ? s_off[t - o] : 0;
    __syncthreads();
    s_off[t] += v;
    __syncthreads();
  }
  if (t < nblk) boff[t] = s_off[t] - q.cnt;
  // integers and (chi^2, row) pairs: the tree's shape plays no part in the result
  for (int o = kMaxPieceBlocks / 2; o > 0; o >>= 1) {
    if (t < o) {
      s_bad[t] += s_bad[t + o];
      s_first[t] = min(s_first[t], s_first[t + o]);
      if (beats(s_chi[t + o], s_best[t + o], s_chi[t], s_best[t])) {
        s_chi[t] = s_chi[t + o];
        s_best[t] = s_best[t + o];
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const int off = s_off[kMaxPieceBlocks - 1];
    const bool have = words[kWHaveBest] != 0;
    // against the rows folded before: only a strictly smaller chi^2 takes over
    const bool take_best = s_best[0] != INT_MAX && (!have || s_chi[0] < best[PS - 1]);
    words[kWPiece] = (unsigned long long)off;
    words[kWUsed] += (unsigned long long)off;
    words[kWBad] += (unsigned long long)s_bad[0];
    words[kWHaveBest] = have || take_best;
    const bool take_pivot = !words[kWHavePivot] && s_first[0] != INT_MAX;
    words[kWPivotNew] = take_pivot;
    if (take_pivot) words[kWHavePivot] = 1;
    s_take[0] = take_best ? s_best[0] : -1;
    s_take[1] = take_pivot ? s_first[0] : -1;
  }
  __syncthreads();
  if (t < PS) {
    if (s_take[0] >= 0) best[t] = row_of(m, s0 + s_take[0])[t];
    if (s_take[1] >= 0) pivot[t] = row_of(m, s0 + s_take[1])[t];
  }
}

// A sample's model as the fold reads it: per Gaussian {amp, x0, y0, a, b, c}, then the
// background -- olpe_eval_kernel's EXACT branch
template <int NSRC>
__device__ __forceinline__ void make_desc(const double *row, int bkgd_mode, double *out) {
  using L = dev::Layout<NSRC>;
  double p[L::NP];
#pragma unroll
  for (int k = 0; k < L::NP; ++k) p[k] = row[k];
  auto q = [&](int k) -> double { return p[k]; };
  const dev::Trig T1 = dev::make_trig<false>(p[L::T1]), T2 = dev::make_trig<false>(p[L::T2]);
  const dev::ModelDesc<NSRC> md = dev::make_model<NSRC>(
      q, dev::make_coef<false>(p[L::S1X], p[L::S1Y], T1),
      dev::make_coef<false>(p[L::S2X], p[L::S2Y], T2), bkgd_mode);
#pragma unroll
  for (int g = 0; g < 2 * NSRC; ++g) {
    out[6 * g] = md.g[g].amp;
    out[6 * g + 1] = md.g[g].x0;
    out[6 * g + 2] = md.g[g].y0;
    out[6 * g + 3] = md.g[g].k.a;
    out[6 * g + 4] = md.g[g].k.b;
    out[6 * g + 5] = md.g[g].k.c;
  }
  out[12 * NSRC] = md.bg;
}

// sweep_exact's pixel (column xj, row yi) of the model d
template <int NSRC>
__device__ __forceinline__ double pixel_model(const double *d, double xj, double yi) {
  constexpr int G = 2 * NSRC;
  double v[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const double xd = xj - d[6 * g + 1];
    const double t1 = d[6 * g + 3] * (xd * xd);
    const double t2 = d[6 * g + 4] * xd;
    const double yd = yi - d[6 * g + 2];
    const double qq = (t1 + t2 * yd) + d[6 * g + 5] * (yd * yd);
    v[g] = d[6 * g] * dev::exp_neg(qq);
  }
  double mod = v[0] + v[1];
#pragma unroll
  for (int s = 1; s < NSRC; ++s) mod = mod + (v[2 * s] + v[2 * s + 1]);
  return mod + d[6 * G];
}

// 4. desc: the usable rows' models at their compact positions
template <int NSRC>
__global__ __launch_bounds__(kThreads) void resid_desc_kernel(RowMap m, long long s0, int ns,
                                                              const int *__restrict__ boff,
                                                              int bkgd_mode,
                                                              double *__restrict__ desc) {
  constexpr int KS = 12 * NSRC + 1;
  __shared__ int s_w[kThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int s = blockIdx.x * kB + t;
  const double *row = row_of(m, s0 + (s < ns ? s : 0));
  const bool ok = s < ns && usable_row<dev::Layout<NSRC>::NP>(row);
  const unsigned long long bal = __ballot(ok);
  if (lane == 0) s_w[wave] = __popcll(bal);
  __syncthreads();
  int pos = boff[blockIdx.x] + __popcll(bal & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += s_w[w];
  if (ok) make_desc<NSRC>(row, bkgd_mode, desc + (size_t)pos * KS);
}

template <int K> __device__ __forceinline__ double bcast_lane(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), K);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), K);
  return __longlong_as_double(((long long)(unsigned)lo) | ((long long)hi << 32));
}

bool finite_params(const double *v, int np) {
  for (int k = 0; k < np; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

}  // namespace
