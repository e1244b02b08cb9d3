// olpe_select.h -- exact order statistics of a device array of doubles by radix select,
// shared by olpe_astrom.hip (np.median) and olpe_phot.hip (percentile brackets).
//
// Values are compared through order-preserving 64-bit keys (okey).  The caller knows the
// extremes kmin / kmax of the keys that count and how many there are (n_in); every key
// outside [kmin, kmax] is ignored, which is how NaN stays out: okey of a positive NaN
// lies past +inf's, and the callers' extremes are taken over numbers only.  The select
// works below the keys' common prefix, one digit of kDigit bits per pass: a pass is one
// read of the array that histograms the digit of the keys whose higher digits equal a
// prefix (per workgroup in LDS, merged with integer atomics), the host picks the bin
// that holds the rank.  Several ranks of one array share a pass for as long as they fall
// into the same bins (select_ranks); the key that follows a found one costs one more
// read (select_next), which is how a neighbouring rank is had without a second descent
// (select_brackets: the pair of ranks around a virtual index).
// Integer work only: the result does not depend on the order of anything.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/olpe.h"
#include "olpe_internal.h"
#include "olpe_reduce.h"

namespace olpe {

constexpr int kSelThreads = 256;     // block size of the two kernels
constexpr int kSelDigit = 11;        // 2048 bins, 8 KiB of LDS
constexpr int kSelBins = 1 << kSelDigit;
constexpr int kSelBlocks = 1024;
constexpr int kSelMaxRanks = 16;

// order-preserving key of a double (negative values below positive ones, -0.0 just
// below +0.0, a positive NaN above +inf) and its inverse
__host__ __device__ __forceinline__ unsigned long long okey(double x) {
  unsigned long long b;
  memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double okey_inv(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  memcpy(&x, &b, 8);
  return x;
}

// one digit of the radix select: the histogram of digit (d >> shift) & (bins - 1) of the
// keys d = okey(x) - kmin <= span whose bits above `pshift` equal `prefix` (all of them
// when !filt).  A key outside [kmin, kmin + span] wraps to d > span or exceeds it.
static __global__ __launch_bounds__(kSelThreads) void select_hist_kernel(
    const double *__restrict__ x, long long n, unsigned long long kmin, unsigned long long span,
    int shift, int bins, int filt, int pshift, unsigned long long prefix,
    unsigned long long *__restrict__ ghist) {
  __shared__ unsigned h[kSelBins];
  for (int i = threadIdx.x; i < kSelBins; i += kSelThreads) h[i] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * kSelThreads + threadIdx.x; i < n;
       i += (long long)gridDim.x * kSelThreads) {
    const unsigned long long d = okey(x[i]) - kmin;
    if (d <= span && (!filt || (d >> pshift) == prefix))
      atomicAdd(&h[(unsigned)(d >> shift) & (bins - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += kSelThreads)
    if (h[i]) atomicAdd(&ghist[i], (unsigned long long)h[i]);
}

// the smallest key above `key` and not above `kmax`
static __global__ __launch_bounds__(kSelThreads) void select_next_kernel(
    const double *__restrict__ x, long long n, unsigned long long key, unsigned long long kmax,
    unsigned long long *__restrict__ out) {
  __shared__ unsigned long long red[kSelThreads];
  unsigned long long m = ~0ull;
  for (long long i = (long long)blockIdx.x * kSelThreads + threadIdx.x; i < n;
       i += (long long)gridDim.x * kSelThreads) {
    const unsigned long long k = okey(x[i]);
    if (k > key && k <= kmax && k < m) m = k;
  }
  m = block_word<kSelThreads, WordMin>(m, red);
  if (threadIdx.x == 0) atomicMin(out, m);
}

inline unsigned select_grid(long long n) {
  const long long b = (n + kSelThreads - 1) / kSelThreads;
  return (unsigned)std::max(1ll, std::min<long long>(b, kSelBlocks));
}

// a rank asked for (k, 0-based among the n_in keys in [kmin, kmax]) and what the select
// found: its key, how many keys lie below that key and how many equal it
struct SelRank {
  long long k = 0;
  unsigned long long key = 0, below = 0, equal = 0;
};

// The order statistics r[0 .. nr) (k ascending, each < n_in) of x[0 .. n) on `stream`;
// d_hist holds kSelBins words.  `passes` counts the reads of x.  Returns when done.
inline int select_ranks(hipStream_t stream, unsigned long long *d_hist, const double *x,
                        long long n, unsigned long long n_in, unsigned long long kmin,
                        unsigned long long kmax, SelRank *r, int nr, int *passes) {
  struct Group {
    unsigned long long prefix, below, count;
    int first, last;               // ranks [first, last)
  };
  if (nr < 1 || nr > kSelMaxRanks) return set_err(OLPE_EINVAL, "radix select of %d ranks", nr);
  for (int i = 0; i < nr; ++i)
    if (r[i].k < 0 || (unsigned long long)r[i].k >= n_in || (i && r[i].k < r[i - 1].k))
      return set_err(OLPE_EINVAL, "radix select: rank %lld of %llu out of order or range",
                     r[i].k, n_in);
  const unsigned long long span = kmax - kmin;
  int pos = 0;
  while (pos < 64 && (span >> pos) != 0) ++pos;            // bits in which the keys differ
  std::vector<Group> cur{{0ull, 0ull, n_in, 0, nr}}, nxt;
  std::vector<unsigned long long> h(kSelBins);
  bool first = true;
  while (pos > 0) {
    const int bits = pos % kSelDigit ? pos % kSelDigit : kSelDigit;
    const int shift = pos - bits;
    nxt.clear();
    for (const Group &g : cur) {
      HIPCHK(hipMemsetAsync(d_hist, 0, kSelBins * 8, stream));
      hipLaunchKernelGGL(select_hist_kernel, dim3(select_grid(n)), dim3(kSelThreads), 0, stream,
                         x, n, kmin, span, shift, 1 << bits, first ? 0 : 1, first ? 0 : pos,
                         g.prefix, d_hist);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(h.data(), d_hist, (size_t)(1 << bits) * 8, hipMemcpyDeviceToHost,
                            stream));
      HIPCHK(hipStreamSynchronize(stream));
      if (passes) ++*passes;
      unsigned long long cum = g.below;
      int i = g.first;
      for (int bin = 0; bin < (1 << bits) && i < g.last; ++bin) {
        if (h[bin] && (unsigned long long)r[i].k < cum + h[bin]) {
          Group s{(g.prefix << bits) | (unsigned long long)bin, cum, h[bin], i, i};
          while (s.last < g.last && (unsigned long long)r[s.last].k < cum + h[bin]) ++s.last;
          i = s.last;
          nxt.push_back(s);
        }
        cum += h[bin];
      }
      if (i < g.last) return set_err(OLPE_EHIP, "radix select: histogram short of its rank");
    }
    cur.swap(nxt);
    pos = shift;
    first = false;
  }
  for (const Group &g : cur)
    for (int i = g.first; i < g.last; ++i) {
      r[i].key = kmin + g.prefix;
      r[i].below = g.below;
      r[i].equal = g.count;
    }
  return OLPE_OK;
}

// the smallest key of x[0 .. n) above `key` and not above `kmax` into *out (all ones if
// there is none); d_word is one device word.  Returns when done.
inline int select_next(hipStream_t stream, unsigned long long *d_word, const double *x,
                       long long n, unsigned long long key, unsigned long long kmax,
                       unsigned long long *out, int *passes) {
  const unsigned long long all = ~0ull;
  HIPCHK(hipMemcpyAsync(d_word, &all, 8, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(select_next_kernel, dim3(select_grid(n)), dim3(kSelThreads), 0, stream, x,
                     n, key, kmax, d_word);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, d_word, 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (passes) ++*passes;
  return OLPE_OK;
}

// The brackets of the order statistics at the virtual indices vidx[0 .. nr) (ascending, each
// in [0, n_in - 1], as np.percentile's (n - 1) p): lo[i] / hi[i] are the keys at ranks
// floor(v) and ceil(v).  One shared descent for the lower ranks; an upper rank that is not a
// copy of its lower one costs one more read.  d_hist as for select_ranks, d_word as for
// select_next; `passes` counts the reads of x.
inline int select_brackets(hipStream_t stream, unsigned long long *d_hist,
                           unsigned long long *d_word, const double *x, long long n,
                           unsigned long long n_in, unsigned long long kmin,
                           unsigned long long kmax, const double *vidx, int nr,
                           unsigned long long *lo, unsigned long long *hi, int *passes) {
  SelRank r[kSelMaxRanks];
  for (int i = 0; i < nr && i < kSelMaxRanks; ++i) r[i].k = (long long)floor(vidx[i]);
  int rc;
  if ((rc = select_ranks(stream, d_hist, x, n, n_in, kmin, kmax, r, nr, passes))) return rc;
  for (int i = 0; i < nr; ++i) {
    lo[i] = hi[i] = r[i].key;
    // keys <= r.key: those below it and its copies
    if (ceil(vidx[i]) != floor(vidx[i]) &&
        (unsigned long long)(r[i].k + 1) >= r[i].below + r[i].equal &&
        (rc = select_next(stream, d_word, x, n, r[i].key, kmax, &hi[i], passes)))
      return rc;
  }
  return OLPE_OK;
}

}  // namespace olpe
