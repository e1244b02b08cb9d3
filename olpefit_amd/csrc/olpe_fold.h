// olpe_fold.h -- what the step-3 fold objects (olpe_astrom, olpe_corner, olpe_resid,
// olpe_acf, olpe_phot, olpe_cov, olpe_lik) share on the host: the device, a stream and an event of
// their own, device buffers, and the one statement of how a fold joins a sampler's stream
// (fold_run).  No device code.
//
// A fold object belongs to a device, not to a sampler context.  It folds a context's last
// launch at most once, asynchronously on that context's stream: the fold runs behind the
// launch and behind whatever the object still has in flight, and the host does not wait.
// `ev` marks the last such fold; the object's own stream (row uploads, finalize) waits
// for it (wait_pending), the host when state is read, added to or reset (drain).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "../../include/olpe.h"
#include "olpe_internal.h"

namespace olpe {

struct FoldBase {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;      // the last fold on a sampler's stream
  bool ev_pending = false;
  const olpe_ctx *last_ctx = nullptr;   // the launch folded last
  long long last_launch = 0;
};

// makes `device` the calling thread's
inline int open_device(int device) {
  if (device < 0) return set_err(OLPE_EINVAL, "device %d (there is no CPU path)", device);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
    (void)hipGetLastError();
    return set_err(OLPE_EHIP, "no HIP device %d (%d visible)", device, ndev);
  }
  HIPCHK(hipSetDevice(device));
  return OLPE_OK;
}

// the object's stream and event, on the current device `device`
inline int fold_open(FoldBase *b, int device) {
  b->device = device;
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&b->ev, hipEventDisableTiming) != hipSuccess)
    return set_err(OLPE_EHIP, "stream / event creation failed");
  return OLPE_OK;
}

// waits for everything in flight, frees `bufs` (null entries allowed), then the event and
// the stream; a half-opened object is fine
inline void fold_close(FoldBase *b, std::initializer_list<void *> bufs) {
  (void)hipSetDevice(b->device);
  if (b->ev_pending) (void)hipEventSynchronize(b->ev);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  for (void *p : bufs)
    if (p) (void)hipFree(p);
  if (b->ev) (void)hipEventDestroy(b->ev);
  if (b->stream) (void)hipStreamDestroy(b->stream);
}

inline int alloc(void **p, size_t bytes, const char *what) {
  if (hipMalloc(p, bytes) != hipSuccess) {
    *p = nullptr;
    (void)hipGetLastError();
    return set_err(OLPE_ENOMEM, "hipMalloc(%zu bytes) for %s", bytes, what);
  }
  return OLPE_OK;
}

// a buffer of at least `bytes` (nothing of the object is in flight when it grows)
inline int grow(void **p, size_t *cap, size_t bytes, const char *what) {
  if (*cap >= bytes) return OLPE_OK;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  int rc = alloc(p, bytes, what);
  if (!rc) *cap = bytes;
  return rc;
}

// the object's own stream waits for its last fold on a sampler's stream
inline int wait_pending(FoldBase *b) {
  if (b->ev_pending) {
    HIPCHK(hipStreamWaitEvent(b->stream, b->ev, 0));
    b->ev_pending = false;
  }
  return OLPE_OK;
}

// everything the object has in flight is done when this returns
inline int drain(FoldBase *b) {
  if (b->ev_pending) {
    HIPCHK(hipEventSynchronize(b->ev));
    b->ev_pending = false;
  }
  HIPCHK(hipStreamSynchronize(b->stream));
  return OLPE_OK;
}

// A fold of context c's last launch: the caller checks its arguments and fold_check (there
// is a launch, and this object has not folded it), refuses what does not fit, sets the
// device and reserves what the launches need; fold_run does the rest.
inline int fold_check(const FoldBase *b, const olpe_ctx *c) {
  if (!c->d_state || !c->launches) return set_err(OLPE_ESTATE, "no sampler launch yet");
  if (b->last_ctx == c && b->last_launch == c->launches)
    return set_err(OLPE_ESTATE, "the last launch's rows are already folded");
  return OLPE_OK;
}

inline void fold_mark(FoldBase *b, const olpe_ctx *c) {
  b->last_ctx = c;
  b->last_launch = c->launches;
}

// the context's main-class stream (olpe_main: behind every sampler launch and moments
// fold); the folds hold the context const, the stream bookkeeping is not part of that
inline hipStream_t main_stream(const olpe_ctx *c) { return olpe_main(const_cast<olpe_ctx *>(c)); }

// The main stream is behind the launch already; this puts it behind whatever the object has
// in flight as well (an earlier fold on another context's stream included: drain() then
// waits for one event only)
inline int fold_enter(FoldBase *b, const olpe_ctx *c) {
  int rc;
  if ((rc = wait_pending(b))) return rc;
  HIPCHK(hipEventRecord(b->ev, b->stream));
  HIPCHK(hipStreamWaitEvent(main_stream(c), b->ev, 0));
  return OLPE_OK;
}

inline int fold_leave(FoldBase *b, const olpe_ctx *c) {
  HIPCHK(hipEventRecord(b->ev, main_stream(c)));
  b->ev_pending = true;
  return OLPE_OK;
}

// The fold's place on the context's main stream: the launch counts as folded from here on,
// rows or none (fold_mark); with anything to do (`any`), launch(main stream) runs between
// fold_enter and fold_leave.  The caller bumps its counters when this returns OLPE_OK.
template <class Launch>
int fold_run(FoldBase *b, const olpe_ctx *c, bool any, Launch launch) {
  fold_mark(b, c);
  if (!any) return OLPE_OK;
  int rc;
  if ((rc = fold_enter(b, c))) return rc;
  if ((rc = launch(main_stream(c)))) return rc;
  return fold_leave(b, c);
}

// reset: the launch folded last may be folded again
inline void fold_forget(FoldBase *b) {
  b->last_ctx = nullptr;
  b->last_launch = 0;
}

}  // namespace olpe
