/*
 * olpe_test.h -- test hooks of libolpe.so.  NOT part of the stable C-ABI (include/olpe.h):
 * the library exports them so that the repository's own tests can drive the failure and
 * hand-off paths on a real GPU; a consumer of the sampler has no use for them.
 */
#ifndef OLPE_TEST_H
#define OLPE_TEST_H

#include "olpe.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Failure paths of the collectives (olpe_comm.hip, olpe_comm_proto.h); persistent until
 * cleared with 0:
 *   1  the moments summary's preparation fails to allocate (OLPE_ENOMEM, before any
 *      collective: it travels in the uniformity check),
 *   2  the local summary launch fails after the check (both rounds still entered),
 *   3  the uniformity check's words fail to reach the device (the poisoned default is
 *      sent instead: every rank fails the check; applies to every collective),
 *   4  round 1's summed words fail to come back (the rank enters round 2 as failed). */
int olpe_moments_fault(olpe_ctx *ctx, int where);

/* Chunk hand-offs that provably wait (on != 0; 0 clears).  In every later launch that
 * cuts walkers into chunks (olpe_last_units > 1), a wave that finishes a walker's first
 * chunk holds its hand-off until some wave is waiting for a hand-off, and the launch runs
 * one workgroup more than the first chunks need, so that a later chunk starts while its
 * predecessor is held: olpe_unit_stats counts at least one wait whatever the dispatch
 * order.  The results are unchanged.  OLPE_EINVAL at launch when the workgroups would
 * not all be resident (too many walkers for the device). */
int olpe_test_hold_handoff(olpe_ctx *ctx, int on);

/* How many of the context's sampler launches so far overlapped their predecessor (olpe.h,
 * "Launch overlap"): started behind the launch before it, its chunk 0 waiting per walker
 * on the predecessor's last hand-off tag, instead of behind the predecessor's end. */
int olpe_test_overlaps(olpe_ctx *ctx, long long *count);

/* Upload chain[W][nrec][PS] into the context's device chain buffer as if a sampler launch
 * had just recorded it: grows the buffer as olpe_run does, sets the launch's row count,
 * counts one launch (so olpe_moments_accumulate and every *_fold_ctx accept it), records
 * the launch's two events on the stream.  The iteration count, state, RNG and counters are
 * untouched.  nrec may be 0.  OLPE_ESTATE before olpe_seed. */
int olpe_test_chain_set(olpe_ctx *ctx, const double *chain, long long nrec);

/* The derivatives dM_p / dtheta_k of the model at the PS-vector vec, without the 1 / err
 * weight and at every pixel, masked or not: planes[P][n][n], through the device expressions
 * of olpe_normal_batch (olpe_normal.hip, pixel_jac), so that a wrong lane-to-pixel map or
 * chain-rule entry of the sums can be told apart per pixel. */
int olpe_test_jacobian(olpe_ctx *ctx, const double *vec, double *planes);

#ifdef __cplusplus
}
#endif
#endif /* OLPE_TEST_H */
