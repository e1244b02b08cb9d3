// olpe_internal.h -- the context object behind the opaque olpe_ctx handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct olpe_ctx {
  int device = 0;
  int n = 0;           // square cutout side
  int nsrc = 2;
  int bkgd_mode = 0;
  int np = 16, ps = 17;
  int eval_mode = 1;   // OLPE_EVAL_FAST (default) / OLPE_EVAL_EXACT
  bool lds_img = true; // cutout + 1/err staged in LDS by the sampler
  int wpb = 0;         // waves per workgroup of the 64x64 LDS sampler (0 = 12)
  // the main-class stream.  Only olpe_main() (below) hands it out: everything but the
  // sampler launches and the moments fold runs on it, behind all of them
  hipStream_t stream = nullptr;
  // Launch overlap (olpe_run).  Sampler launches alternate between two
  // streams by parity, so that launch k+1 can take the CUs launch k's tail frees; each
  // parity has its own queue counter (d_queue[0] / [5]) and base, hold word and chain
  // buffer.  The moments fold of a launch runs on that launch's stream.
  hipStream_t sstream[2] = {nullptr, nullptr};
  int par = 0;                       // parity of the last sampler launch
  hipEvent_t ev_tail[2] = {};        // the last work enqueued on sstream[p]
  hipEvent_t ev_fold = nullptr;      // end of the last moments fold
  hipEvent_t ev_main = nullptr;      // the main-class work a launch or fold must follow
  bool pend = false;                 // sampler-stream work the main stream has not waited on
  bool main_dirty = false;           // main-class work enqueued since the last launch
  bool overlap_on = true;            // OLPE_OVERLAP
  bool prev_queue = false;           // the last launch ran the unit queue ...
  long long prev_W = 0;              // ... over this many walkers ...
  unsigned prev_tag = 0;             // ... and its last chunks publish this tag
  unsigned long long *prev_qptr = nullptr;   // its queue counter and that counter's base
  unsigned long long prev_qbase = 0;         // (the gate in front of an overlapped launch)
  int prev_slot = -1;                // its slot in ev[] (-1: no launch to follow)
  long long overlaps = 0;            // launches that overlapped (olpe_test_overlaps)
  unsigned long long qbase2[2] = {0, 0};
  double *d_chain2[2] = {nullptr, nullptr};
  size_t chain_cap2[2] = {0, 0};
  // start/stop events of the last kRing sampler launches (olpe_kernel_times), one slot
  // more so that the oldest one's predecessor is still there; ev_ovl: the launch
  // overlapped its predecessor, whose end event then bounds its time from below
  static constexpr int kRing = 64;
  static constexpr int kSlots = kRing + 1;
  hipEvent_t ev[kSlots][2] = {};
  bool ev_ovl[kSlots] = {};
  long long launches = 0;
  double2 *d_DE = nullptr;   // [n*n] {data as f64, 1/err}, {0,0} where masked (EXACT)
  double2 *d_DW = nullptr;   // [n*n] {data/err, 1/err}, {0,0} where masked (FAST)
  // walker ensemble
  int W = 0;
  bool seeded = false;
  long long count = 0;
  double *d_state = nullptr;     // [W][ps]
  uint32_t *d_tries = nullptr;   // [W][np]
  uint32_t *d_acc = nullptr;     // [W][np]
  uint32_t *d_mt = nullptr;      // [W][624]
  int *d_mtpos = nullptr;        // [W]
  double *d_gauss = nullptr;     // [W]
  int *d_hasg = nullptr;         // [W]
  long long *d_done = nullptr;   // [W]
  // last launch's chain / trace (d_chain, chain_cap: d_chain2 / chain_cap2 [par])
  double *d_chain = nullptr;
  size_t chain_cap = 0;
  long long chain_rows = 0;
  double *d_trace = nullptr;
  size_t trace_cap = 0;
  int trace_on = 0;
  long long trace_iters = 0;
  // scratch for olpe_model / olpe_chi2_batch
  double *d_scratch = nullptr, *d_scratch2 = nullptr;
  size_t scratch_cap = 0, scratch2_cap = 0;
  // walker queue of the sampler (one 64-bit counter per launch parity; each launch takes
  // W + its waves from its own, so no reset between launches): qbase2[p] = that
  // counter's value at launch
  unsigned long long *d_queue = nullptr;
  bool queue_on = true;
  int n_cu = 0;
  // work units (choose_units): walkers cut into chunks handed between waves through
  // uflag[W]; utag = the last launch's tag base (+16 per launch)
  unsigned *d_uflag = nullptr;
  unsigned utag = 0;
  int units_override = 0;   // OLPE_UNITS
  bool hold_handoff = false; // test hook (olpe_test_hold_handoff)
  int last_units = 1;       // chunks per walker of the last launch (olpe_last_units)
  bool units_used = false;  // some launch handed chunks between waves (check_units)
  double wait_limit_s = 30; // hand-off wait limit of the last launch (unit_wait)
  double wait_ticks_override = 0;  // OLPE_WAIT_TICKS (tests of the time-out path)
  int balance = -1;         // progress balancing (-1: launch_gibbs_t picks)
  int ring_wpb = 12;        // 128x128 FAST: the lockstep LDS-ring sampler's waves per
                            // workgroup, 0 = the L2-resident sampler (OLPE_RING)
  int stagger = 0;          // wave start offsets (always 0; see GibbsArgs)
  // jump widths (apf_step2.py:234; 3body :220-238): d_widths [np] is what a launch reads,
  // d_wdef [np] the defaults the device filled in from olpe.hip's tables (the tuner's
  // clamps are multiples of them)
  double *d_widths = nullptr, *d_wdef = nullptr;
  uint32_t logmask = 0;         // bit j: parameter j is log-proposed (Layout::LOGMASK)
  // the tuner's session (olpe_tune.hip): d_tune holds the sums now and before, then the log
  void *d_tune = nullptr;
  bool tune_on = false;
  int tune_k = 0;               // steps taken in this session
  double tune_target = 0, tune_gain = 0;
  // whole-run moments of the recorded rows (olpe_moments.hip): running mean / M2 per
  // walker and column, [ps][W]; mom_n rows folded per walker; mom_folded = the launch
  // whose rows were folded last (a launch is folded at most once)
  double *d_mmean = nullptr, *d_mm2 = nullptr;
  size_t mom_cap = 0;
  long long mom_n = 0;
  long long mom_folded = 0;
  double *d_mpart = nullptr;    // partial sums of olpe_moments_local
  size_t mpart_cap = 0;
  int mom_fault = 0;            // test hook (olpe_moments_fault, include/olpe_test.h): 1 =
                                // the preparation's allocation fails, 2 = the summary launch
                                // fails, 3 = the check words' send fails, 4 = round 1's
                                // read-back fails
  // RCCL communicator (olpe_comm.hip)
  void *comm = nullptr;
  int nranks = 1, rank = 0;
  double *d_gather = nullptr;   // receive buffer of olpe_comm_allgather_chain
  size_t gather_cap = 0;
  size_t gather_limit = 0;      // its byte limit (olpe_comm_gather_limit; 0 = none)
  long long *d_check = nullptr; // the collectives' words: the uniformity check's, then the
                                // poisoned defaults (olpe_comm_setup, called by olpe_create,
                                // so that joining a communicator allocates nothing)
  double comm_timeout_s = 600;  // bound on every wait for the other ranks (olpe_comm_timeout)
  bool comm_aborted = false;    // the communicator was aborted after a timeout / RCCL error
};

namespace olpe {
int set_err(int code, const char *fmt, ...);
}
// a failed HIP call ends the calling function with OLPE_EHIP and the call's text
#define HIPCHK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return ::olpe::set_err(OLPE_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
// The main-class stream: first makes it wait for every sampler launch and moments fold
// still outstanding on the sampler streams, and notes that the next launch has to follow
// what the caller enqueues (olpe.hip).  Every use of the context's stream outside
// olpe_run and olpe_moments_accumulate goes through it.
hipStream_t olpe_main(olpe_ctx *c);
// the stream of the last sampler launch, for the moments fold: behind the previous fold
// and any main-class work; olpe_fold_done records the fold's end
int olpe_fold_stream(olpe_ctx *c, hipStream_t *s);
int olpe_fold_done(olpe_ctx *c);
void olpe_comm_release(olpe_ctx *c);
// the default jump widths into c->d_widths (with_base: into c->d_wdef too), a launch on
// the context's stream (olpe.hip, where the default tables live)
int olpe_widths_defaults(olpe_ctx *c, bool with_base);
// the collectives' word buffer with its poisoned defaults (olpe_comm.hip; olpe_create)
int olpe_comm_setup(olpe_ctx *c);
// the buffers (and zeroing) of the per-column sums (olpe_moments.hip); then the sums over
// this context's walkers into d_out[2 ..], launches only
int olpe_moments_prepare(olpe_ctx *c);
int olpe_moments_local(olpe_ctx *c, const double *d_centre, double *d_out);
// What olpe_detnull.hip takes from an olpe_detect (olpe_detect.hip; not part of the C-ABI):
// its shape, and with a vector (host, PS - 1 parameters) that vector evaluated as
// olpe_detect_point does, synchronously, the pointers then being the object's slot-0 tables
// [os^2][2n - 1][2n - 1], its staged cutout [n^2], and the vector's Q [G] and sigma_A [G]
// planes, valid until the object's next call.  vec NULL: the shape only, no GPU call.
struct olpe_detect;
struct olpe_detect_view {
  int device, n, os, gs, ps;
  size_t tabs;
  const double *tab;
  const double2 *DE;
  const double *Q;
  const double *sigma;
};
__attribute__((visibility("hidden"))) int olpe_detect_view_at(olpe_detect *d, const double *vec,
                                                              olpe_detect_view *v);
