// olpe_store.h -- the sample store olpe_astrom and olpe_phot are built on: planes [cap][W]
// of derived samples on the device (rows outer, walkers inner -- the order of
// step3.load_chains), sample (row r, walker w) of plane q at q * cap * W + r * W + w, filled
// row by row by the object's fold kernel from a sampler's chain or from host rows; with the
// buffers the reductions over the filled prefix and the radix select (olpe_select.h) work in.
// Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/olpe.h"
#include "olpe_fold.h"
#include "olpe_internal.h"

namespace olpe {

struct SampleStore : FoldBase {
  int variant = 2;            // sources
  int ps = 17;
  long long W = 0, cap = 0;   // walkers, row capacity per walker
  long long rows = 0;         // rows folded per walker
  double *d_store = nullptr;  // the planes, cap * W samples each
  double *d_part = nullptr;   // reduction partials
  double *d_out = nullptr;    // reduction results
  unsigned long long *d_words = nullptr;  // [0] unusable rows; the others are the object's
  unsigned long long *d_hist = nullptr;   // [kSelBins]
  double *d_stage = nullptr;  // upload staging of fold_rows
  size_t stage_cap = 0;
};

// what a store can be made for; `group`: walkers per grid row (blockIdx.y) of the fold kernel
inline int store_geometry(long long walkers, long long row_cap, int group) {
  if (walkers < 1 || row_cap < 1 || walkers > 65535ll * group || row_cap > 0x7fffffffll ||
      walkers > (1ll << 40) / row_cap)
    return set_err(OLPE_EINVAL, "walkers %lld x row capacity %lld", walkers, row_cap);
  return OLPE_OK;
}

// refuses `more` rows per walker that do not fit
inline int store_room(const SampleStore *a, long long more) {
  if (a->rows + more <= a->cap) return OLPE_OK;
  return set_err(OLPE_ESTATE, "sample store full: %lld + %lld rows per walker, capacity %lld",
                 a->rows, more, a->cap);
}

inline double *store_plane(const SampleStore *a, int q) {
  return a->d_store + (size_t)q * a->W * a->cap;
}

// fold_rows: nrows > 0 host rows of per_row doubles through the staging buffer, in pieces of
// at most 64 MiB.  piece(r0, nr) gives the host address of rows r0 .. r0 + nr as they travel;
// launch(nr) folds them from d_stage into rows a->rows .. on the object's stream.
template <class Piece, class Launch>
int store_upload(SampleStore *a, long long nrows, long long per_row, Piece piece, Launch launch) {
  HIPCHK(hipSetDevice(a->device));
  int rc;
  if ((rc = wait_pending(a))) return rc;
  const long long chunk = std::max(1ll, std::min(nrows, (long long)(1 << 23) / per_row));
  if ((rc = grow((void **)&a->d_stage, &a->stage_cap, (size_t)(chunk * per_row) * 8,
                 "the row upload")))
    return rc;
  for (long long r0 = 0; r0 < nrows; r0 += chunk) {
    const long long nr = std::min(chunk, nrows - r0);
    HIPCHK(hipMemcpyAsync(a->d_stage, piece(r0, nr), (size_t)(nr * per_row) * 8,
                          hipMemcpyHostToDevice, a->stream));
    if ((rc = launch(nr))) return rc;
    HIPCHK(hipStreamSynchronize(a->stream));   // the piece's host memory and d_stage are reused
    a->rows += nr;
  }
  return OLPE_OK;
}

inline int store_rows(const SampleStore *a, long long *rows) {
  if (!a || !rows) return set_err(OLPE_EINVAL, "NULL argument");
  *rows = a->rows;
  return OLPE_OK;
}

// the filled prefix of plane q to host dst (the caller has waited for the folds)
inline int store_read(const SampleStore *a, int q, double *dst) {
  const size_t n = (size_t)a->rows * a->W;
  if (n) HIPCHK(hipMemcpy(dst, store_plane(a, q), n * 8, hipMemcpyDeviceToHost));
  return OLPE_OK;
}

}  // namespace olpe
