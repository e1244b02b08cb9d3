/*
 * olpe.h -- C-ABI of libolpe.so, the MI355X (gfx950) implementation of the
 * apf_step2 Gibbs/Metropolis-Hastings hot path of logan-pearce/olpefit.
 *
 * The reference has no FFI: its seam is the call sequence at
 * apf_step2.py:312-318 (build_analytical_model -> chi_squared -> accept_reject)
 * driven by the loop at :300-365, module-level functions reading the globals
 * xsize/ysize.  Each entry point below names the reference code it replaces.
 *
 * Conventions
 *  - Every int-returning call returns OLPE_OK (0) or a negative OLPE_E* code and
 *    never aborts; olpe_last_error() gives a thread-local message.
 *  - The caller owns every host buffer.  A context owns the device copies of the
 *    image / inverse-sigma map and of the walker ensemble (state, counters, RNG).
 *  - One context is bound to one HIP device (no CPU path: device < 0 or a host
 *    without a GPU is an error).  Calls on one context are not thread-safe;
 *    separate contexts (one per GPU) may be used concurrently.
 *  - Parameter vectors use the reference layout: P = 16 (nsrc 2,
 *    apf_step2.py:108) or 19 (nsrc 3, 3body/apf_step2_3body.py:266-288)
 *    proposable parameters followed by the chi^2 slot, PS = P + 1 doubles.
 */
#ifndef OLPE_H
#define OLPE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OLPE_OK 0
#define OLPE_EINVAL (-1)  /* bad argument */
#define OLPE_EHIP (-2)    /* HIP runtime error / no GPU */
#define OLPE_ENOMEM (-3)  /* device allocation failed */
#define OLPE_ESTATE (-4)  /* call out of order (e.g. run before seeding) */
#define OLPE_ECOMM (-5)   /* RCCL error */
#define OLPE_EIO (-6)     /* file write failed */

#define OLPE_DTYPE_F32 0
#define OLPE_DTYPE_F64 1

#define OLPE_EVAL_EXACT 0 /* one exp per pixel-Gaussian, reference op order */
#define OLPE_EVAL_FAST 1  /* separable exps + cross-term recurrence (default) */

typedef struct olpe_ctx olpe_ctx;

/* Library version (major*10000 + minor*100 + patch). */
int olpe_version(void);
/* Number of visible HIP devices (0 on a host without a GPU). */
int olpe_device_count(int *count);
/* Free / total device memory of a HIP device (sizes a run's launches so that the
 * per-launch chain buffer fits; OLPE_EHIP without a GPU). */
int olpe_device_mem(int device, long long *free_bytes, long long *total_bytes);
/* PCI bus id ("dddd:bb:dd.f") of a HIP device into buf (len >= 16): a multi-process run
 * checks that its ranks' devices are distinct GPUs whatever each process sees as device
 * 0..n-1 (bench.py, one process per GPU).  Build-specific: no reference counterpart. */
int olpe_device_pci_id(int device, char *buf, int len);
/* Thread-local message describing the last error. */
const char *olpe_last_error(void);

/* Create a context for one N x N cutout.  Replaces the setup at apf_step2.py:160-237
 * (the environment knob OLPE_WPB, a tuning experiment, must be 8, 12 or 16 and fit the
 * LDS, else OLPE_EINVAL with the byte count):
 *   image      ny*nx row-major, float32 (image_dtype OLPE_DTYPE_F32, BITPIX -32) or
 *              float64; promoted to f64 exactly as ``data - model`` does (:135).
 *   pois2      |D| Poisson term squared, same dtype as image, rounded as the
 *              reference rounds it (``np.sqrt(np.abs(image))**2``, :207-210).
 *   readnoise2 readnoise**2 (f64), :197-204.  err = sqrt(readnoise2 + pois2) (:210).
 *   mask       u8, 1 = excluded (``np.ma.masked_greater(image, 0.8*satlevel)``, :188);
 *              may be NULL (nothing masked).
 *   ny == nx   the reference is square-only (:237 swaps the axes and :123 fails to
 *              broadcast otherwise); ny != nx is OLPE_EINVAL.
 *   nsrc       2 (apf_step2.py) or 3 (3body/apf_step2_3body.py).
 *   bkgd_mode  0 = reference quirk, background fill p[12] (apf_step2.py:119-120);
 *              1 = fill p[9] (the dead code at :126-132).  Ignored for nsrc 3.
 *   device     HIP ordinal (>= 0). */
int olpe_create(const void *image, int image_dtype, const void *pois2, double readnoise2,
                const uint8_t *mask, int ny, int nx, int nsrc, int bkgd_mode, int device,
                olpe_ctx **out);
void olpe_destroy(olpe_ctx *ctx);
/* Select OLPE_EVAL_FAST (default) or OLPE_EVAL_EXACT for every evaluation of ctx. */
int olpe_set_eval_mode(olpe_ctx *ctx, int mode);

/* build_analytical_model (apf_step2.py:106-124; 3body :106-125): one PS-vector ->
 * N*N f64 model image.  Test hook. */
int olpe_model(olpe_ctx *ctx, const double *params, double *model_out);
/* chi_squared(image_nanmask, build_analytical_model(p), err) (apf_step2.py:314-316,
 * :134-137) for W parameter vectors [W][PS] -> chi2_out[W]. */
int olpe_chi2_batch(olpe_ctx *ctx, const double *params, int W, double *chi2_out);
/* Gauss-Newton sums of explicit parameter vectors (no reference line: the reference
 * has no optimiser; model of apf_step2.py:106-124, residual of :134-137).  With
 * r_p = (D_p - M_p) / err_p and J_pk = (dM_p / dtheta_k) / err_p over the usable pixels of
 * the cutout (masked pixels contribute exact zeros):  chi2 = sum r^2,  grad[k] = sum J_pk r_p
 * (so d chi^2 / d theta_k = -2 grad[k]),  jtj[k][l] = sum J_pk J_pl.  The model is the EXACT
 * one whatever the context's eval mode.  In bkgd_mode 0 of the 2-source layout p[12] is
 * sigma_x of the wide set and the background: its column is the sum of both.  A vector's
 * outputs are the same bits for any W, any place in the batch and every repeat.  A vector
 * with a non-finite parameter, or whose model is not finite at a usable pixel, gets NaN in
 * all its outputs; the rest of the batch is untouched.  Waits for the result. */
int olpe_normal_batch(olpe_ctx *ctx, const double *params /*[W][PS]*/, int W,
                      double *chi2 /*[W]*/, double *grad /*[W][P]*/,
                      double *jtj /*[W][P][P], symmetric, both halves written*/);

/* --- walker ensemble (device resident) ------------------------------------------ */
/* np.random.seed(seeds[w]) for W walkers (init_genrand semantics)
 * and allocate the ensemble.  The reference seeds nothing (OS entropy per rank); the
 * build seeds per walker so runs are reproducible and GPU-count independent. */
int olpe_seed(olpe_ctx *ctx, const uint32_t *seeds, int W);
/* Upload walker state [W][PS] (params + chi^2) and counters tries/accepts [W][P]
 * (apf_step2.py:273-289; counters as the reference's float arrays, :276).
 * tries/accepts may be NULL (zeros).  If chi^2 slots are NaN they are NOT recomputed:
 * call olpe_chi2_batch first, as :283-289 does. */
int olpe_state_set(olpe_ctx *ctx, const double *state, const double *tries,
                   const double *accepts);
int olpe_state_get(olpe_ctx *ctx, double *state, double *tries, double *accepts);
/* Run n_iters Gibbs iterations of every walker (the loop body apf_step2.py:300-333)
 * asynchronously on the context's stream.  The ensemble keeps a global iteration
 * count c; the state after iteration c is recorded when c >= burn_in and
 * (c - burn_in) % record_stride == 0 (apf_step2.py:342-351 with stride 1) into the
 * device chain buffer of this launch (read with olpe_chain_read).  record_stride 0
 * records nothing.  accept_min > 0 tracks, per walker, the first c at which every
 * parameter has been tried accept_min times (the loop condition :300); read it with
 * olpe_done_at.  *nrec_out (may be NULL) = rows recorded per walker by this launch.
 * n_iters per call must be < 2^31 (OLPE_EINVAL otherwise; split long runs). */
int olpe_run(olpe_ctx *ctx, long long n_iters, long long burn_in, int record_stride,
             long long accept_min, long long *nrec_out);
/* Copy the last launch's chain [W][nrec][PS] to the host (synchronises). */
int olpe_chain_read(olpe_ctx *ctx, double *chain_out);
/* Iteration count of the ensemble (iterations completed so far). */
int olpe_count(olpe_ctx *ctx, long long *count);
int olpe_count_reset(olpe_ctx *ctx, long long count);
/* Per walker: first count c with min(tries) >= accept_min, or -1. */
int olpe_done_at(olpe_ctx *ctx, long long *done_at);
/* One-shot form of the loop: upload state/tries/accepts for W
 * walkers (already seeded with olpe_seed), reset the count to 0, run, download.
 * chain_out [W][nrec][PS] may be NULL. */
int olpe_run_gibbs(olpe_ctx *ctx, double *state, double *tries, double *accepts, int W,
                   long long n_iters, long long burn_in, int record_stride,
                   double *chain_out);

/* RNG state for resume/parity: mt_state [W][625] = 624 key words + position,
 * gauss_cache [W][2] = {has_gauss, cached deviate}. */
int olpe_rng_get(olpe_ctx *ctx, uint32_t *mt_state, double *gauss_cache);
int olpe_rng_set(olpe_ctx *ctx, const uint32_t *mt_state, const double *gauss_cache);
/* Test hook: draw n values per walker from the ensemble streams.
 * kind 0 = raw u32 (out as uint32 [W][n]); 1 = rand() f64; 2 = gauss f64;
 * 3 = randint(0, P) as f64.  Advances the streams. */
int olpe_rng_stream(olpe_ctx *ctx, int kind, int n, void *out);

/* Per-iteration trace of the next olpe_run (test hook): on != 0 enables it.
 * olpe_trace_read: [W][n_iters][6] f64 = {r, proposed value, chi^2 proposal, dice,
 * p_accept, accepted}. */
int olpe_trace_enable(olpe_ctx *ctx, int on);
int olpe_trace_read(olpe_ctx *ctx, double *out);

/* Launch overlap.  Consecutive olpe_run launches of one context run on two sampler
 * streams, alternately, and a launch may start while its predecessor's last walkers still
 * run: each of its walkers then waits, on the device, for that walker's end in the
 * predecessor.  This happens when both launches run the sampler's unit queue over the same
 * walkers, nothing but olpe_moments_accumulate was called on the context between them, no
 * trace is recorded, and the environment variable OLPE_OVERLAP is not 0; otherwise a launch
 * waits for its predecessor's end.  olpe_moments_accumulate follows the launch it folds and
 * the fold before it.  Every other call that touches the device runs behind all launches
 * and folds enqueued so far, and the next launch behind it: results and their order are
 * those of one stream.  A process with one context opens three hardware queues. */

/* Wait for everything the context has enqueued. */
int olpe_sync(olpe_ctx *ctx);
/* Duration (ms, HIP events on the launch's stream) of the last sampler launch. */
int olpe_last_kernel_ms(olpe_ctx *ctx, double *ms);
/* Durations of the last n sampler launches (oldest first; n <= 64 and <= launches so
 * far): launches can be queued back to back and timed afterwards.  A launch's time runs to
 * its end from its start or, where it overlapped its predecessor, from that launch's end
 * if that is later: back-to-back launches then sum to the time they took together. */
int olpe_kernel_times(olpe_ctx *ctx, int n, double *ms_out);
/* Chunks per walker of the last sampler launch (1 = whole walkers; > 1 when the launch
 * cut each walker's iterations into chunks to fill the resident waves).
 * Results do not depend on it.  Build-specific: no reference counterpart. */
int olpe_last_units(olpe_ctx *ctx, int *units);
/* Chunk hand-offs that had to wait since the context was created: out[0] = waits,
 * out[1] = total wave-time spent waiting (ns).  Diagnostics; build-specific. */
int olpe_unit_stats(olpe_ctx *ctx, long long *out);

/* --- jump widths (apf_step2.py:234; 3body/apf_step2_3body.py:220-238) --------------
 * The reference's one tuning knob: the scale of proposal() (:63-65, loc + w gauss()) and
 * of logproposal() (:66-70, 10**(log10 loc + w gauss()), w in dex), one per proposable
 * parameter, edited by hand in the source.  Here each context carries its own [P] on the
 * device; the defaults are the reference's. */
/* The largest width a log-proposed parameter takes.  The FAST form of logproposal is
 * cur * e^(w g ln 10), the exponential by the table exp (ExpTab) once |w g ln 10| >=
 * 1/16; ExpTab is tested on [-1000, 710] and returns inf beyond 710.  The polar method
 * forms g = x sqrt(-2 ln(r2) / r2) with r2 = x1^2 + x2^2 and x1, x2 multiples of 2^-52, so
 * |g| <= sqrt(-2 ln r2) <= sqrt(208 ln 2) = 12.0073 (r2 >= 2^-104).  Hence the exponent
 * stays inside the domain for w <= 710 / (12.0073 ln 10) = 25.68; the entry point takes
 * up to 25 (|w g ln 10| <= 691.2). */
#define OLPE_LOG_WIDTH_MAX 25.0
/* Replace the context's widths with w[P]; w == NULL restores the defaults.  Ordered on the
 * context's stream without a host wait (w is copied before the call returns): every launch
 * enqueued afterwards runs with the new widths, none enqueued before.  OLPE_EINVAL, with
 * the widths unchanged, for an entry that is not finite and > 0 and for a log-proposed
 * parameter (lognorm, apf_step2.py:217; 3body :295) above OLPE_LOG_WIDTH_MAX. */
int olpe_widths_set(olpe_ctx *ctx, const double *w);
/* The widths in force once the context's stream has drained into out[P] (synchronises). */
int olpe_widths_get(olpe_ctx *ctx, double *out);

/* --- acceptance-rate tuner of the jump widths --------------------------------------
 * What a user of the reference does by hand between runs (read {rank}_acceptance.txt,
 * apf_step2.py:362-365, edit :234), done on the device between launches from the
 * ensemble's own counters, without a host round trip.  Build-specific.
 * olpe_tune_begin: needs 0 < target < 1, gain > 0 and gain * target < 1 (so that every
 * factor below is positive), else OLPE_EINVAL; OLPE_ESTATE before olpe_seed.  Sets the
 * step count k = 0 and takes the baseline: the 64-bit integer sums over walkers of
 * tries[.][j] and accepts[.][j].
 * olpe_tune_step: enqueues on the context's stream, without synchronising,
 *   1. the same sums again (integer: exact in any order);
 *   2. the signed deltas dT_j, dA_j against the previous sums, which they replace;
 *   3. k <- k + 1;
 *   4. for every j with dT_j > 0:  a = double(dA_j) / double(dT_j),
 *      f = 1 + g_k (a - target) with g_k = gain / sqrt(k) (formed on the host),
 *      w_j <- min(max(w_j f, default_j / 1024), default_j * 64); a parameter with
 *      dT_j <= 0 keeps its width exactly.  Each operation is one correctly rounded IEEE
 *      double operation in this order (no contraction, no fast division);
 *   5. appends (dT, dA, the new widths) to a device log of OLPE_TUNE_LOG steps.
 * OLPE_ESTATE without olpe_tune_begin, or with the log full.
 * olpe_tune_get: synchronises; *steps = k, and the log oldest first into dT, dA, widths
 * ([k][P] each; any may be NULL; OLPE_TUNE_LOG rows are always enough).  The log of an
 * ended session stays readable until the next olpe_tune_begin.
 * olpe_tune_end: ends the session; the widths stay as they are. */
#define OLPE_TUNE_LOG 256
int olpe_tune_begin(olpe_ctx *ctx, double target, double gain);
int olpe_tune_step(olpe_ctx *ctx);
int olpe_tune_get(olpe_ctx *ctx, int *steps, long long *dT, long long *dA, double *widths);
int olpe_tune_end(olpe_ctx *ctx);

/* --- chain files (apf_step2.py:342-360; 3body/apf_step2_3body.py:381-399) ---------
 * Host-only (no GPU needed).  Rows are formatted as the reference's csv.writer writes
 * a list of float rows: repr() of each value (shortest round-trip digits, fixed
 * notation for decimal exponents -4..15, 'nan'/'inf'), ',' between fields, "\r\n"
 * after each row.  nan_row != 0 prepends the all-NaN row the reference seeds
 * total_parameters with (apf_step2.py:278-279). */
/* Format rows [nrows][ncols] into out (cap bytes; out may be NULL to query the size):
 * *len_out = bytes of the text. */
int olpe_csv_format(const double *rows, long long nrows, int ncols, int nan_row, char *out,
                    size_t cap, size_t *len_out);
/* Write nfiles chain files: file i gets chains[i][nrows][ncols] (the per-walker
 * {rank}_finalarray_mpi.csv), from `threads` writer threads (0 = one per core). */
int olpe_csv_write_chains(const char *const *paths, const double *chains, int nfiles,
                          long long nrows, int ncols, int nan_row, int threads);

/* Streaming form of the same files.  The reference rewrites each file every 10
 * iterations (apf_step2.py:355-360), so a killed run leaves its chains on disk; the
 * build appends each launch's rows instead: rows [0, nrows) of
 * chains[i][rows_per_file][ncols] are appended to file i (created if absent; no NaN
 * row -- write it first with olpe_csv_write_chains and nrows 0).  sizes_out [nfiles]
 * (may be NULL) receives each file's size in bytes after the append: a checkpoint
 * records it, and a resumed run truncates the file back to it. */
int olpe_csv_append_chains(const char *const *paths, const double *chains, int nfiles,
                           long long rows_per_file, long long nrows, int ncols, int threads,
                           long long *sizes_out);

/* Step 3's read of the same files (apf_step3.py:169-186: np.genfromtxt per walker
 * file, the walkers collated as columns).  olpe_csv_shape: *rows = non-blank lines,
 * *cols = fields of the first line (step 3 takes the length from walker 0's file).
 * olpe_csv_read_chains: nfiles files of nrows x ncols each, rows [skip, nrows) into
 * out[nrows - skip][nfiles][ncols] (skip = step 3's additional_burnin, :190-205), parsed
 * from `threads` threads (0 = one per core); values equal genfromtxt's bit for bit
 * (correctly rounded; empty field = NaN).  A file of another shape is OLPE_EINVAL
 * naming the file (the reference fails assigning it into its [length, ncor] arrays). */
int olpe_csv_shape(const char *path, long long *rows, int *cols);
int olpe_csv_read_chains(const char *const *paths, int nfiles, long long nrows, int ncols,
                         long long skip, double *out, int threads);

/* Step 2's acceptance files (apf_step2.py:362-365: str(total_accept / total_tries), NumPy's
 * print of a float64 array).  Host-only.  olpe_acceptance_write: file i gets
 * accepts[i][np] / tries[i][np] as NumPy prints it, from `threads` threads (0 = one per
 * core), for the rows NumPy prints in fixed notation (all values finite, the non-zero
 * ones in [1e-4, 1e8) within a factor 1000 of each other): done[i] = 1; done[i] = 0 for
 * the rows left to the caller (scientific notation, NaN).  olpe_acceptance_format: the
 * text for x[0..n) (*len_out = 0 when x is outside that range; out may be NULL to query
 * the size). */
int olpe_acceptance_format(const double *x, int n, char *out, size_t cap, size_t *len_out);
int olpe_acceptance_write(const char *const *paths, const double *accepts, const double *tries,
                          int nfiles, int np, int threads, unsigned char *done);

/* --- multi-GPU (RCCL over xGMI), SURVEY.md §8(e) ---------------------------------
 * The reference's ranks meet at a per-iteration comm.barrier() (apf_step2.py:338); the
 * build's ranks meet only in these end-of-run collectives.  No rank is left waiting:
 * every call first all-reduces a word set (shard sizes, ranges, local failures), and a
 * rank decides whether to enter the data collective only from that agreed verdict (a
 * rank whose words cannot reach the device sends a poisoned default that fails the
 * check everywhere); the moments summary runs both all-reduce rounds on every rank and
 * decides success from their summed status words.  A failure inside a collective (a dead
 * peer) is bounded by olpe_comm_timeout: a rank that waits longer aborts its
 * communicator (OLPE_ECOMM; later collectives OLPE_ESTATE until olpe_comm_init). */
/* 128-byte RCCL unique id, created on rank 0 and shared by the host. */
int olpe_comm_unique_id(uint8_t *id128);
/* Join the communicator (a non-blocking RCCL communicator: its later waits are bounded by
 * olpe_comm_timeout).  The set-up itself returns once every rank has arrived -- RCCL's
 * bootstrap, not boundable here -- so callers meet on their own host group, with a
 * timeout, to share the id first (bench.py).  RCCL's own rank count and rank are checked
 * against nranks / rank. */
int olpe_comm_init(olpe_ctx *ctx, const uint8_t *id128, int nranks, int rank);
/* Seconds a collective may wait for the other ranks before it aborts the communicator and
 * returns OLPE_ECOMM; 0 = no bound.  Default 600.  Build-specific. */
int olpe_comm_timeout(olpe_ctx *ctx, double seconds);
/* RCCL's own view of the communicator: ncclCommCount / ncclCommUserRank (OLPE_ESTATE
 * without one).  Build-specific. */
int olpe_comm_info(olpe_ctx *ctx, int *nranks, int *rank);
/* All-gather the walker states of every rank: out [nranks*W][PS] (rank-major; equal W
 * on every rank, checked). */
int olpe_comm_allgather_state(olpe_ctx *ctx, double *out);
/* Chain concatenation (north star: "RCCL all-gather over xGMI only for the final chain
 * concatenation"; the reference leaves one {rank}_finalarray_mpi.csv per MPI rank,
 * apf_step2.py:355-360): all-gather walkers [w0, w0+wn) of the last launch's chain
 * from every rank into out [nranks][wn][nrec][PS] (rank-major; host memory, or NULL to
 * leave the gathered range in the context's device buffer, e.g. to time the
 * collective alone).  Gathering a large ensemble range by range bounds both the device
 * receive buffer and the host buffer by the range.  *nrec_out (may be NULL) = nrec.
 * Every rank must call with the same range and have the same W and nrec (checked:
 * OLPE_EINVAL on every rank otherwise).  The receive buffer is allocated before that
 * check and its outcome travels with it: a rank that cannot allocate it (or whose
 * olpe_comm_gather_limit it exceeds) makes the call OLPE_ENOMEM on every rank. */
int olpe_comm_allgather_chain(olpe_ctx *ctx, long long w0, long long wn, double *out,
                              long long *nrec_out);
/* Byte limit of the chain gather's device receive buffer (nranks x range bytes; 0 = no
 * limit, the default): a memory budget for the gather, like bench.py's --gather-mib. */
int olpe_comm_gather_limit(olpe_ctx *ctx, long long bytes);
/* Posterior summary over every rank from the whole-run moments (olpe_moments_*): two
 * all-reduces (sum), the pooled mean first, then the deviations of the walkers' means
 * about it.  out[OLPE_MOMENTS_LEN(PS, P)] as for olpe_moments_summary, over all ranks'
 * walkers, with centre = the pooled mean (out[2 + k] / out[1]).  Every rank must have
 * folded the same number of rows (checked: OLPE_EINVAL on every rank otherwise); the
 * walker counts may differ (a sum needs no equal shards).
 * Without olpe_comm_init it summarises this context alone.  Every local allocation (and
 * the zeroing of unfolded moments) happens before the uniformity check and its failure
 * travels in it (OLPE_ENOMEM on every rank); past the check every rank enters both
 * all-reduces whatever happened locally, a failure summed into a status word, so all
 * ranks return an error together (this rank's own, or OLPE_ECOMM naming how many other
 * ranks failed) -- except a rank that fails only to read round 2's sums back, which
 * returns its own error while its peers succeed. */
int olpe_comm_allreduce_moments(olpe_ctx *ctx, double *out);

/* --- whole-run posterior moments ----------------------------
 * apf_step3.py reads every chain file (:169-186) to compute per-parameter means, sigmas
 * and the Gelman-Rubin PSRF / RC (:258-278).  Those need, per walker w and column k,
 * only the walker's mean and sum of squared deviations M2 over its rows, which the
 * device keeps for every row the walker recorded: the summary then needs neither the
 * chain files nor a chain gather.  Rows = what the chain files hold after step 3's
 * default additional_burnin = 1 (the NaN seed row) -- every recorded row. */
/* Fold the last launch's recorded rows into the running (mean, M2) of every walker and
 * column (async; once per launch: OLPE_ESTATE if this launch was folded already).
 * olpe_seed starts a new run (no rows folded). */
int olpe_moments_accumulate(olpe_ctx *ctx);
int olpe_moments_reset(olpe_ctx *ctx);
/* *n = rows folded per walker; mean / m2 [W][PS] (either may be NULL).  _set restores a
 * checkpoint (n = 0: nothing folded; mean / m2 may then be NULL). */
int olpe_moments_get(olpe_ctx *ctx, long long *n, double *mean, double *m2);
int olpe_moments_set(olpe_ctx *ctx, long long n, const double *mean, const double *m2);
/* Per-column sums over this context's walkers (no communication):
 *   out[0] = n rows per walker, out[1] = walkers W,
 *   out[2 + k]          = sum_w mean_w[k]                         (k < PS)
 *   out[2 + PS + k]     = sum_w M2_w[k]
 *   out[2 + 2*PS + k]   = sum_w (mean_w[k] - centre[k])^2         (0 if centre is NULL)
 *   out[2 + 3*PS + j]   = sum_w tries_w[j], out[2 + 3*PS + P + j] = sum_w accepts_w[j]
 *                                                                 (j < P, whole run)
 * Per-parameter mean = out[2+k] / W; step 3's np.std over all rows =
 * sqrt((out[2+PS+k] + n * out[2+2PS+k]) / (n W)) with centre = that mean; GR's within
 * term = out[2+PS+k] / (n W), its between sum = out[2+2PS+k] (step3.summary_from_moments). */
#define OLPE_MOMENTS_LEN(ps, np) (2 + 3 * (ps) + 2 * (np))
int olpe_moments_summary(olpe_ctx *ctx, const double *centre, double *out);

/* --- separation / position-angle posteriors ----------------
 * What step 3 is run for: the median and scatter of the companion's separation (mas) and
 * position angle (deg) and its delta RA / Dec, apf_step3.py:211-256, :283-343, :401-450
 * (3body/apf_step3_3body.py:247-288, :315-390, :450-518).  The chain rows are turned into
 * (sep, pa) samples and reduced on the device, so a large run needs neither its chain
 * files nor a host pass over them.  An olpe_astrom belongs to a device, not to a sampler
 * context: step 3 uses it on chains read from files as well.  Calls on one object are not
 * thread-safe.  Not covered: computing deltaR (the name resolver, the AltAz transform and
 * atm_corr, :348-391) and medians over several objects.  The photometry (:452-511) is
 * olpe_phot's, below. */
typedef struct olpe_astrom olpe_astrom;
/* Doubles per pair of olpe_astrom_finalize's output:
 *   [0] np.median(sep_corrected), [1] np.std(sep_corrected)              (:436)
 *   [2] np.median(pa_angle),      [3] np.std(pa_angle)                   (:437)
 *   [4] RA = -np.mean(RA), [5] np.std(RA), [6] Dec = np.mean(Dec), [7] np.std(Dec)
 *       (:446-450; variant 3 swaps sin / cos and does not negate, 3body :508-518)
 *   [8] np.mean(pa) as :401 sees it (after :340-341), [9] the branch taken (OLPE_ASTROM_*),
 *   [10] samples (rows x walkers), [11] 1 if :340-341 added 360
 *   [12..15] np.mean of the de-distorted x / y of the primary, x / y of the companion
 *       (:250-253; what :365-366 feeds to the refraction term). */
#define OLPE_ASTROM_LEN 16
#define OLPE_ASTROM_BELOW_180 0        /* :402 with mean(pa) >= 90: + 180 (:413) */
#define OLPE_ASTROM_BELOW_0 1          /* :402 with mean(pa) < 90 (:415) */
#define OLPE_ASTROM_ABOVE_360 2        /* :425 (3body :481): + 360 */
#define OLPE_ASTROM_ABOVE_180 3        /* :427 (3body :483): + 180 */
#define OLPE_ASTROM_ABOVE_0 4          /* :430 (3body :486) */
#define OLPE_ASTROM_BELOW_PER_SAMPLE 5 /* 3body :462: + 180 where pa_angle < 0 */
/* The set-up of :211-253 and :283-337 for one frame:
 *   variant        2 (apf_step3.py: one pair) or 3 (3body: b - a and c - a)
 *   ps, pair_cols  doubles per chain row; per pair the columns {x, y of the primary, x, y
 *                  of the companion} (variant 2: {0,1,2,3}; 3: {0,1,2,3, 0,1,4,5}), npairs
 *                  = variant - 1
 *   x_dist/y_dist  the distortion look-up tables (:218-231), f64 [tab_ny][tab_nx], copied
 *                  to the device; both NULL: no correction (the tables are not shipped)
 *   xdiff/ydiff    the index offsets of :241-242
 *   pixscale       mas per pixel (:224 / :231); rotation_angle :300 / :302; rotcorr :334,
 *                  added only if use_rotcorr != 0 (ROTMODE 'vertical angle', :309)
 *   walkers, row_cap  the store holds row_cap rows of every walker (2 doubles per walker,
 *                  row and pair).
 * A sample whose position is non-finite or whose table index falls outside the table
 * (where the reference raises, or wraps a negative index) is never used as an index: it
 * is counted, and olpe_astrom_finalize fails.  Invalid arguments are OLPE_EINVAL before
 * any GPU call; a failed allocation is OLPE_ENOMEM naming its bytes. */
int olpe_astrom_create(int device, int variant, int ps, const int *pair_cols, int npairs,
                       const double *x_dist, const double *y_dist, int tab_ny, int tab_nx,
                       int xdiff, int ydiff, double pixscale, double rotation_angle,
                       double rotcorr, int use_rotcorr, long long walkers, long long row_cap,
                       olpe_astrom **out);
void olpe_astrom_destroy(olpe_astrom *a);
/* :211-256, :283-304, :337 for the rows of ctx's last launch, read from its device chain
 * (async on the context's stream, no host copy).  Once per launch (OLPE_ESTATE if this
 * launch was folded already); OLPE_ESTATE if the store would overflow. */
int olpe_astrom_fold_ctx(olpe_astrom *a, olpe_ctx *ctx);
/* The same for host rows [nrows][walkers][ps] as step 3 collates them (:169-205,
 * step3.load_chains); only the position columns are uploaded. */
int olpe_astrom_fold_rows(olpe_astrom *a, const double *rows, long long nrows);
/* Rows folded per walker so far. */
int olpe_astrom_rows(olpe_astrom *a, long long *rows);
/* :340-341, :401-450 (3body :383-386, :450-518) over every folded sample, with the
 * differential refraction deltaR (mas; :391) and PARANTEL (:393) given: out
 * [npairs][OLPE_ASTROM_LEN].  Every sum runs over the store in a fixed order, so the
 * result does not depend on how the rows were split over folds.  The store then holds
 * (sep_corrected, pa_angle): one finalize per object.  OLPE_EINVAL, with the count, if
 * any sample was unusable (see olpe_astrom_create). */
int olpe_astrom_finalize(olpe_astrom *a, double delta_r, double parantel, double *out);
/* After finalize: the device's sep_corrected into out[0 .. n) and pa_angle into
 * out[n .. 2n), n = rows x walkers, sample (row r, walker w) at r * walkers + w. */
int olpe_astrom_samples(olpe_astrom *a, int pair, double *out);

/* --- corner-plot histograms (apf_step3.py:603-643) -------------------------------------
 * The reference ends by flattening every parameter chain into corner.corner(...,
 * show_titles=True, plot_contours=True) (apf_step3.py:603-643; 3body/apf_step3_3body.py
 * likewise): a 1-D histogram per column, a 2-D histogram per pair of columns and each
 * title's 16 / 50 / 84 % quantiles.  An olpe_corner counts the data behind that figure on
 * the device: h1 [ncols][nb1] (fine bins, which the quantile brackets are read from) and
 * h2 [npairs][nb2][nb2] over the pairs (i, j), i < j, in lexicographic order, bin index
 * of column i first, as np.histogram2d(x = column i, y = column j).  Counts are 64-bit and
 * additive: they stream launch by launch without a sample store and merge across objects,
 * ranks and checkpoints by addition; they do not depend on how the rows were split.
 * The bin rule is NumPy's: x is in bin k of a column iff e[k] <= x < e[k+1], x equal to
 * the last edge is in the last bin, anything else (NaN and +-inf included) is in no bin.
 * A sample counts in h1[c] iff column c has a bin, in h2[p] iff both columns of the pair
 * have one; n counts every sample folded.  An olpe_corner belongs to a device, not to a
 * sampler context.  Calls on one object are not thread-safe.  Not covered: the drawing,
 * contour levels, exact quantiles (they need a sample store). */
typedef struct olpe_corner olpe_corner;
/* apf_step3.py:603-643: the bin edges of every column, edges1 [ncols][nb1 + 1] for the 1-D
 * histograms and edges2 [ncols][nb2 + 1] for the 2-D ones, each column's finite and
 * strictly increasing (any spacing).  2 <= ncols <= 24, 2 <= nb1 <= 4096, 2 <= nb2 <= 64.
 * Anything else is OLPE_EINVAL (naming the column) before any GPU call, as is a
 * configuration whose smallest tile does not fit a workgroup's LDS (naming the bytes). */
int olpe_corner_create(int device, int ncols, const double *edges1, int nb1,
                       const double *edges2, int nb2, olpe_corner **out);
/* Frees the object of apf_step3.py:603-643's counts (waits for its folds in flight). */
void olpe_corner_destroy(olpe_corner *h);
/* apf_step3.py:603-643 for the rows of ctx's last launch, read from its device chain
 * (async on the context's stream, no host copy; ncols == PS).  Once per launch:
 * OLPE_ESTATE if this launch was folded already; OLPE_EINVAL for a context of another
 * device or PS. */
int olpe_corner_fold_ctx(olpe_corner *h, olpe_ctx *ctx);
/* apf_step3.py:603-643 for host rows [nsamples][ncols], uploaded in bounded pieces. */
int olpe_corner_fold_rows(olpe_corner *h, const double *rows, long long nsamples);
/* The counts so far (apf_step3.py:603-643): *n samples folded, h1 [ncols][nb1],
 * h2 [npairs][nb2][nb2]; any of the three may be NULL.  Waits for the folds in flight. */
int olpe_corner_get(olpe_corner *h, unsigned long long *n, unsigned long long *h1,
                    unsigned long long *h2);
/* Adds another object's, rank's or checkpoint's counts of the same shape
 * (apf_step3.py:603-643 over the union of their rows). */
int olpe_corner_add(olpe_corner *h, unsigned long long n, const unsigned long long *h1,
                    const unsigned long long *h2);
/* Zeroes the counts (apf_step3.py:603-643 starts over); the edges stay. */
int olpe_corner_reset(olpe_corner *h);

/* --- posterior model and residual images (apf_step2.py:106-124) ------------------------
 * The picture the reference's README opens with (model_residuals_all.png: data, model,
 * residual), over the whole ensemble: every folded sample's build_analytical_model
 * (apf_step2.py:106-124; 3body/apf_step2_3body.py:106-125) is evaluated on the device in
 * the EXACT operation order, whatever the context's eval mode, and folded per pixel into
 * the shifted sums S1 = sum (M_s - R), S2 = sum (M_s - R)^2 about a pivot image R, the
 * model of a pivot vector.  The state (counts, pivot, S1, S2, best row) is additive across
 * folds, objects, ranks and checkpoints whose pivots are equal.  A row with a non-finite
 * parameter (the all-NaN seed row of a chain file) contributes to nothing and is counted
 * in n_bad.  The best sample is the usable row with the smallest chi^2 column (NaN never
 * wins; the earliest in fold order on a tie).  No result depends on the grid, the CU
 * count or the tile height; the same sequence of folds gives the same bits.  Calls on one
 * object are not thread-safe.  Not covered: the drawing, a factorised (FAST) fold, a
 * collective over the state, photometry (per-pixel chi^2 over all samples: olpe_lik below). */
typedef struct olpe_resid olpe_resid;
#define OLPE_RESID_PLANES 7
/* olpe_resid_finalize's planes [OLPE_RESID_PLANES][n][n], D the data, err as apf_step2.py
 * :210, chi_squared's residual as :134-137:
 *   [0] mean of the models over the samples        [1] their np.std (ddof 0)
 *   [2] model of the best sample                   [3] D - [2]      [4] (D - [2]) / err
 *   [5] D - [0]                                    [6] (D - [0]) / err
 * [3..6] are NaN at the pixels the context staged as masked.  Its scalars: */
#define OLPE_RESID_SCALARS 8
#define OLPE_RESID_USED 0      /* samples folded (usable) */
#define OLPE_RESID_BAD 1       /* unusable rows met */
#define OLPE_RESID_PIXELS 2    /* unmasked pixels */
#define OLPE_RESID_BEST_CHI2 3 /* the best row's chi^2 column */
#define OLPE_RESID_SUM4 4      /* sum of plane 4 squared: that chi^2 evaluated here (:134-137) */
#define OLPE_RESID_SUM6 5      /* sum of plane 6 squared */
#define OLPE_RESID_MAX4 6      /* max |plane 4| ... */
#define OLPE_RESID_MAX4_AT 7   /* ... and its pixel, row * n + column */
/* Copies ctx's staged cutout (apf_step2.py:176-210: data, 1/err, mask) device to device and
 * takes its side, sources, bkgd_mode and device; independent of ctx afterwards.  pivot: a
 * parameter vector (its PS - 1 parameters are read, all finite), or NULL: the first usable
 * row folded becomes the pivot.
 * OLPE_RESID_ROWS=8|16 picks the fold kernel's tile height (A/B; no result depends on it).
 * OLPE_EINVAL, naming the bytes, for a frame whose partial sums per block exceed 1 GiB. */
int olpe_resid_create(olpe_ctx *ctx, const double *pivot, olpe_resid **out);
/* Frees the object of apf_step2.py:106-124's images (waits for its folds in flight). */
void olpe_resid_destroy(olpe_resid *r);
/* apf_step2.py:106-124 for rows 0, row_step, ... of walkers 0, walker_step, ... of ctx's
 * last launch, read from its device chain in place, walker-major (async on the context's
 * stream, no copy).  Once per launch: OLPE_ESTATE if this launch was folded already;
 * OLPE_EINVAL for a context of another device, side, nsrc or bkgd_mode. */
int olpe_resid_fold_ctx(olpe_resid *r, olpe_ctx *ctx, int row_step, int walker_step);
/* apf_step2.py:106-124 for host rows [nsamples][PS], uploaded in bounded pieces. */
int olpe_resid_fold_rows(olpe_resid *r, const double *rows, long long nsamples);
/* The state (apf_step2.py:106-124 summed): samples used, unusable rows, pivot [PS], S1 and
 * S2 [n*n] each, best row [PS]; any may be NULL; pivot / best are NaN while there is none.
 * Waits for the folds in flight. */
int olpe_resid_get(olpe_resid *r, long long *n, long long *n_bad, double *pivot, double *s1,
                   double *s2, double *best);
/* Adds another object's, rank's or checkpoint's state (apf_step2.py:106-124 over the union
 * of their rows).  OLPE_EINVAL if the pivots' parameters differ in any bit, unless this
 * object holds no sample yet: it then adopts the incoming pivot.  This object's rows count
 * as folded first: the incoming best row wins only with a strictly smaller chi^2. */
int olpe_resid_add(olpe_resid *r, long long n, long long n_bad, const double *pivot,
                   const double *s1, const double *s2, const double *best);
/* Empties the state (apf_step2.py:106-124 starts over); a pivot given at create stays. */
int olpe_resid_reset(olpe_resid *r);
/* The planes and scalars above (apf_step2.py:106-137 per plane) from the state, which it
 * leaves as it is: more folds and another finalize may follow.  OLPE_ESTATE with no
 * usable sample, or when no usable sample's chi^2 is a number. */
int olpe_resid_finalize(olpe_resid *r, double *planes, double *scalars);

/* --- pointwise deviance, WAIC and DIC (apf_step2.py:106-124, :134-148) -------------------
 * The reference's chi_squared (apf_step2.py:134-148; 3body/apf_step2_3body.py:134-148) is
 * one number per vector and its column is only plotted; the sampler's target is
 * exp(-chi^2 / 2) (:144-148), so a pixel's log likelihood is log p(D_i | theta) = -x_i / 2
 * + k_i with x_i = ((D_i - M_i) / err_i)^2 and k_i = -log err_i - log(2 pi) / 2.  An
 * olpe_lik evaluates every folded sample's build_analytical_model (:106-124; 3body
 * :106-125) in the EXACT operation order, whatever the context's eval mode, forms t = (D -
 * M) * (1 / err) on the staged operands and x = t * t, and keeps per pixel, about the plane
 * c = x of a pivot vector: A1 = sum (x - c), A2 = sum (x - c)^2, and the log-sum-exp pair
 * m = min x, L = sum exp(-(x - m) / 2) (empty: +inf, 0).  Pairs merge by m' = min(m_a, m_b),
 * L' = L_a exp(-(m_a - m') / 2) + L_b exp(-(m_b - m') / 2), the minimum's factor exactly 1,
 * an empty side skipped.  k_i is left out of the planes (it cancels in every comparison on
 * the same data) and reported summed as OLPE_LIK_LOG_NORM.  Unusable rows, the best row and
 * the pivot follow olpe_resid's rules.  A sample whose t is not finite at a pixel (a model
 * that overflows) is not dropped at that pixel as np.ma (:134-137) would drop it: the
 * pixel's sums become non-finite, finalize writes NaN into its planes, leaves it out of
 * every total and counts it in OLPE_LIK_POISONED.  No result depends on the grid, the CU
 * count or the tile height; the same sequence of folds gives the same bits.  Calls on one
 * object are not thread-safe.  Not covered: PSIS-LOO, a factorised (FAST) fold, a
 * collective over the state, priors (the reference has none), plots. */
typedef struct olpe_lik olpe_lik;
#define OLPE_LIK_PLANES 7
/* olpe_lik_finalize's planes [OLPE_LIK_PLANES][n][n] over the ns samples folded
 * (apf_step2.py:134-137 per pixel and sample); NaN at masked and at poisoned pixels: */
#define OLPE_LIK_PLANE_MEAN_DEV 0 /* c + A1 / ns */
#define OLPE_LIK_PLANE_STD_DEV 1  /* sqrt(max((A2 - A1^2 / ns) / ns, 0)): np.std of x, ddof 0 */
#define OLPE_LIK_PLANE_LPPD 2     /* log(L / ns) - m / 2 */
#define OLPE_LIK_PLANE_P_WAIC 3   /* (A2 - A1^2 / ns) / (ns - 1) / 4; 0 when ns = 1 */
#define OLPE_LIK_PLANE_ELPD 4     /* [2] - [3] */
#define OLPE_LIK_PLANE_DEV_BEST 5 /* x of the best row */
#define OLPE_LIK_PLANE_DEV_AT 6   /* x of theta_hat; NaN without one */
/* Its scalars; N = PIXELS - POISONED, P the number of parameters: */
#define OLPE_LIK_SCALARS 17
#define OLPE_LIK_USED 0           /* samples folded (usable) */
#define OLPE_LIK_BAD 1            /* unusable rows met */
#define OLPE_LIK_PIXELS 2         /* unmasked pixels */
#define OLPE_LIK_POISONED 3       /* of those, pixels with a non-finite sum */
#define OLPE_LIK_LPPD 4           /* sum of plane 2 */
#define OLPE_LIK_P_WAIC 5         /* sum of plane 3 */
#define OLPE_LIK_ELPD_WAIC 6      /* sum of plane 4 */
#define OLPE_LIK_WAIC 7           /* -2 x [6] */
#define OLPE_LIK_SE_ELPD 8        /* sqrt(N var_i(plane 4)), ddof 1 */
#define OLPE_LIK_P_WAIC_HIGH 9    /* pixels with plane 3 > 0.4 */
#define OLPE_LIK_MEAN_DEVIANCE 10 /* sum of plane 0 */
#define OLPE_LIK_REDUCED 11       /* [10] / (N - P) */
#define OLPE_LIK_DEVIANCE_BEST 12 /* sum of plane 5 */
#define OLPE_LIK_DEVIANCE_AT 13   /* sum of plane 6: D(theta_hat) */
#define OLPE_LIK_P_D 14           /* [10] - [13] */
#define OLPE_LIK_DIC 15           /* [13] + 2 x [14] */
#define OLPE_LIK_LOG_NORM 16      /* sum of k_i over the unmasked pixels */
/* Copies ctx's staged cutout (apf_step2.py:176-210: data, 1/err, mask) device to device and
 * takes its side, sources, bkgd_mode and device; independent of ctx afterwards.  pivot: a
 * parameter vector (its PS - 1 parameters are read, all finite), or NULL: the first usable
 * row folded becomes the pivot.
 * OLPE_LIK_ROWS=4|8 picks the fold kernel's tile height (A/B; no result depends on it).
 * OLPE_EINVAL, naming the bytes, for a frame whose partials per block exceed 1 GiB. */
int olpe_lik_create(olpe_ctx *ctx, const double *pivot, olpe_lik **out);
/* Frees the object of apf_step2.py:134-148's pixel terms (waits for its folds in flight). */
void olpe_lik_destroy(olpe_lik *l);
/* apf_step2.py:106-124 and :134-137 for rows 0, row_step, ... of walkers 0, walker_step, ...
 * of ctx's last launch, read from its device chain in place, walker-major (async on the
 * context's stream, no copy).  Once per launch: OLPE_ESTATE if this launch was folded
 * already; OLPE_EINVAL for a context of another device, side, nsrc or bkgd_mode. */
int olpe_lik_fold_ctx(olpe_lik *l, olpe_ctx *ctx, int row_step, int walker_step);
/* apf_step2.py:106-124 and :134-137 for host rows [nsamples][PS], uploaded in bounded
 * pieces. */
int olpe_lik_fold_rows(olpe_lik *l, const double *rows, long long nsamples);
/* The state (apf_step2.py:134-137 per pixel, summed over the samples): samples used,
 * unusable rows, pivot [PS], A1, A2, m and L [n*n] each, best row [PS]; any may be NULL;
 * pivot / best are NaN while there is none.  Waits for the folds in flight. */
int olpe_lik_get(olpe_lik *l, long long *n, long long *n_bad, double *pivot, double *a1,
                 double *a2, double *m, double *lsum, double *best);
/* Merges another object's, rank's or checkpoint's state (apf_step2.py:134-137 over the
 * union of their rows) by the rule above.  OLPE_EINVAL if the pivots' parameters differ in
 * any bit, unless this object holds no sample yet: it then adopts the incoming pivot.  This
 * object's rows count as folded first: the incoming best row wins only with a strictly
 * smaller chi^2. */
int olpe_lik_add(olpe_lik *l, long long n, long long n_bad, const double *pivot,
                 const double *a1, const double *a2, const double *m, const double *lsum,
                 const double *best);
/* Empties the state (apf_step2.py:134-137 starts over); a pivot given at create stays. */
int olpe_lik_reset(olpe_lik *l);
/* x of one parameter vector (apf_step2.py:134-137 before the sum; PS - 1 parameters read):
 * plane [n][n], NaN at masked pixels. */
int olpe_lik_point(olpe_lik *l, const double *vec, double *plane);
/* The planes and scalars above (apf_step2.py:134-148 per pixel) from the state, which it
 * leaves as it is.  theta_hat: the vector of DIC's D(theta_hat) (step 3 passes the column
 * means), or NULL: plane 6 and scalars 13 - 15 are NaN.  OLPE_ESTATE with no usable sample,
 * or when no usable sample's chi^2 is a number. */
int olpe_lik_finalize(olpe_lik *l, const double *theta_hat, double *planes, double *scalars);

/* --- autocorrelation times of the chains (apf_step3.py:582-601) --------------------------
 * The reference draws every walker's trace of every parameter (apf_step3.py:582-601) and
 * additional_burnin, accept_min and the record stride are chosen from the picture.  An
 * olpe_acf holds the numbers behind an integrated autocorrelation time per column.  A
 * series is one walker's values of one column over one contiguous run of recorded rows
 * x[0 .. N-1]; with the pivot p = x[0], y[t] = (x[t] - p) - mean_t(x[t] - p).  The state is,
 * per column c and for the max_lag L given at create,
 *     C[c][k] = sum over series  sum_{t=0}^{N-k-1} y[t] y[t+k],   k = 0 .. L
 * (the biased lag sum, no 1 / (N - k) factor, pooled over the series; a lag k >= N adds
 * exactly 0), and three counters: n values per column folded, series, and skipped -- a
 * series with a non-finite value in any column is left out whole and counted (a chain
 * file's NaN seed row).  The state is additive over launches, objects, ranks and
 * checkpoints; tau = 2 sum_{k<=M} C[k]/C[0] - 1 and n / tau are host arithmetic on it.
 * Every sum runs in an order fixed by the input's shape: the same call on the same input
 * gives the same bits, whatever the device or grid.  An olpe_acf belongs to a device, not to
 * a sampler context.  Calls on one object are not thread-safe.  Not covered: lags across
 * launch boundaries, per-walker tau, an FFT form, a collective over the state. */
typedef struct olpe_acf olpe_acf;
/* apf_step3.py:582-601: 1 <= ncols <= 24; max_lag a multiple of 64 with 64 <= max_lag <=
 * 1024.  Anything else is OLPE_EINVAL, naming the value, before any GPU call.
 * OLPE_ACF_TILE=64..512 (a multiple of 64) sets the fold kernel's time tile (a test knob:
 * results agree to rounding, not to the bit, across tiles). */
int olpe_acf_create(int device, int ncols, int max_lag, olpe_acf **out);
/* Frees the object of apf_step3.py:582-601's sums (waits for its folds in flight). */
void olpe_acf_destroy(olpe_acf *h);
/* apf_step3.py:582-601 for ctx's last launch: each walker's recorded rows of that launch
 * are one series, read from the device chain in place (async on the context's stream, no
 * host copy; ncols == PS).  Once per launch: OLPE_ESTATE if this launch was folded already;
 * OLPE_EINVAL for a context of another device or PS. */
int olpe_acf_fold_ctx(olpe_acf *h, olpe_ctx *ctx);
/* apf_step3.py:582-601 for host rows: nwalkers series of nrows rows, walker-major
 * [nwalkers][nrows][ncols] (time_major 0) or time-major [nrows][nwalkers][ncols] (1, step
 * 3's chains), uploaded as they lie (no transposition) in pieces of whole series of at
 * most 256 MiB.  A single series larger than that is OLPE_EINVAL, naming its bytes: fold
 * it as shorter runs, each its own series. */
int olpe_acf_fold_rows(olpe_acf *h, const double *rows, long long nwalkers, long long nrows,
                       int time_major);
/* The state so far (apf_step3.py:582-601): *n, *series, *skipped and C_out [ncols][max_lag
 * + 1]; any may be NULL.  Waits for the folds in flight. */
int olpe_acf_get(olpe_acf *h, unsigned long long *n, unsigned long long *series,
                 unsigned long long *skipped, double *C_out);
/* Adds another object's, rank's or checkpoint's state (apf_step3.py:582-601 over the union
 * of their series).  OLPE_EINVAL, naming both, if its ncols or max_lag differ. */
int olpe_acf_add(olpe_acf *h, int ncols, int max_lag, unsigned long long n,
                 unsigned long long series, unsigned long long skipped, const double *C_in);
/* Zeroes the state (apf_step3.py:582-601 starts over). */
int olpe_acf_reset(olpe_acf *h);

/* --- photometry posteriors (apf_step3.py:452-511; the model of apf_step2.py:78-124) ----
 * How bright the companion is relative to the star, with its uncertainty, and the PSF's
 * width: what the reference's photometry block (apf_step3.py:452-511; 3body
 * /apf_step3_3body.py:520-569) takes from the image and from 100 rows, taken from every
 * chain row instead.  In build_analytical_model (apf_step2.py:78-124; 3body :78-125) every
 * source shares ampratio q, the widths sx, sy, sx2, sy2, the angles and the amplitude
 * offset b (p[9]; 3body p[12]), so source k integrates to F_k = 2 pi (A_k - b) [(1 - q) sx
 * sy + q sx2 sy2] and the flux ratio of companion k to the primary is (A_k - b) / (A_0 - b).
 * An olpe_phot turns chain rows into Q = 2 (nsrc - 1) + 5 planes of samples on the device,
 * stored [rows][walkers] as the astrometry samples are, in this order:
 *   per companion k = 1 .. nsrc - 1:  flux_ratio_k = (A_k - b) / (A_0 - b),
 *                                     dmag_k = -2.5 log10(flux_ratio_k)
 *   flux_primary      F_0, counts px^2
 *   fwhm_major        2.355 max(sx, sy) pixscale, mas (what apf_step3.py:463-469 means to
 *                     take; what it takes is photometry.reference_fwhm's, on the host)
 *   fwhm_minor        2.355 min(sx, sy) pixscale
 *   fwhm_wide_major   2.355 max(sx2, sy2) pixscale
 *   core_fraction     (1 - q) sx sy / [(1 - q) sx sy + q sx2 sy2]
 * The operation order is stated in olpe_phot.hip; all but log10 is exact IEEE arithmetic.
 * A row is unusable if a column it reads is non-finite, if A_0 - b <= 0 or if a width is
 * <= 0: it stores NaN in every plane and is counted once.  A companion with A_k - b <= 0
 * keeps its ratio and has a NaN dmag_k.  NaN takes part in no statistic, so every plane has
 * its own count.  An olpe_phot belongs to a device, not to a sampler context.  Calls on one
 * object are not thread-safe.  Not covered: the aperture S/N of apf_step3.py:476-511 (per
 * image, not per sample: photometry.aperture_snr on the host), magnitudes on a
 * photometric system, a checkpoint of the store, a collective over it. */
typedef struct olpe_phot olpe_phot;
/* Doubles per plane of olpe_phot_finalize's output for nprobs probabilities:
 *   [0] n, the samples that are not NaN  [1] np.mean  [2] np.std (ddof 0; exactly 0 where
 *   all n are one value)  [3] min  [4] max  [5] the reads of the plane the select made
 *   [6 + 2 j], [7 + 2 j] the order statistics floor((n - 1) p_j) and ceil((n - 1) p_j) of
 *   the n samples (what np.percentile interpolates between, apf_step3.py:435-437's
 *   np.median being p = 0.5).  With n = 0 everything but [0] and [5] is NaN. */
#define OLPE_PHOT_LEN(nprobs) (6 + 2 * (nprobs))
/* The set-up for one frame of apf_step3.py:452-470's numbers: variant 2 (apf_step2.py:
 * 78-97's columns: A at 6, 7, q 8, b 9, widths 10-13) or 3 (3body :78-98: A at 8-10, q 11,
 * b 12, widths 13-16); ps doubles per chain row; pixscale mas per pixel (:224 / :231); the
 * store holds row_cap rows of walkers walkers (8 Q bytes each).  Invalid arguments are
 * OLPE_EINVAL before any GPU call; a capacity the device cannot hold is OLPE_ENOMEM naming
 * its bytes. */
int olpe_phot_create(int device, int variant, int ps, double pixscale, long long walkers,
                     long long row_cap, olpe_phot **out);
/* Frees the samples of apf_step3.py:452-470's columns (waits for its folds in flight). */
void olpe_phot_destroy(olpe_phot *p);
/* The planes (apf_step2.py:78-124's model, apf_step3.py:463-469's FWHM) for rows 0,
 * row_step, 2 row_step, ... of ctx's last launch, read from its device chain in place
 * (async on the context's stream, no host copy).  Once per launch: OLPE_ESTATE if this
 * launch was folded already, and if the store would overflow (nothing is folded then and
 * the launch stays unfolded); OLPE_EINVAL for a context of another device, walker count,
 * PS or source count. */
int olpe_phot_fold_ctx(olpe_phot *p, olpe_ctx *ctx, int row_step);
/* The same (apf_step2.py:78-124, apf_step3.py:463-469) for host rows [nrows][walkers][ps]
 * as step 3 collates them (apf_step3.py:169-205, step3.load_chains), uploaded whole in
 * pieces of at most 64 MiB.  OLPE_ESTATE if the store would overflow. */
int olpe_phot_fold_rows(olpe_phot *p, const double *rows, long long nrows);
/* Rows folded per walker so far (len(sigmax) of apf_step3.py:458). */
int olpe_phot_rows(olpe_phot *p, long long *rows);
/* Unusable rows so far (the NaN seed row of apf_step2.py:278-279 is one per walker).
 * Waits for the folds in flight. */
int olpe_phot_unusable(olpe_phot *p, long long *n);
/* The summary of every plane (np.mean / np.std as apf_step3.py:470 takes them, the order
 * statistics np.median of :435-437 is made of) for probs[0 .. nprobs) in [0, 1], nprobs <=
 * 16: out [Q][OLPE_PHOT_LEN(nprobs)].  Every sum runs over the store in a fixed order, so
 * the result does not depend on how the rows were split over folds; the select is exact.
 * The store is left as it is: more folds and another finalize may follow.  OLPE_ESTATE
 * with no row folded. */
int olpe_phot_finalize(olpe_phot *p, const double *probs, int nprobs, double *out);
/* One plane's samples (apf_step3.py:469's FWHM array and its like) into out[0 .. n), n =
 * rows x walkers, sample (row r, walker w) at r * walkers + w.  Waits for the folds in
 * flight. */
int olpe_phot_samples(olpe_phot *p, int plane, double *out);
/* Empties the store and the unusable count (apf_step3.py:452-470 starts over); the launch
 * folded last may be folded again. */
int olpe_phot_reset(olpe_phot *p);

/* --- parameter covariance: the cross-column sums (apf_step3.py:603-643) -----------------
 * The reference's corner figure (apf_step3.py:603-643) shows every pair of columns as a
 * scatter and gives no number for it.  An olpe_cov holds what every two-column question is
 * a function of: about a fixed pivot p [ncols], with d = x - p per row,
 *     n, skipped      rows folded and rows left out
 *     S1[j]    = sum d_j
 *     S2[j][k] = sum d_j d_k      the full symmetric matrix, its triangles bit-equal
 * and, created with walkers > 0, per walker w its row count nw[w] and S1w[w][j] = its sum of
 * d_j.  A row with a non-finite value in any column is left out whole and counted once: it
 * enters no sum and no nw.  mean = p + S1 / n, cov = (S2 - S1 S1^T / n) / (n - 1); the
 * correlation, the error ellipse, the conditional widths and the multivariate Gelman-Rubin
 * statistic are host arithmetic on the state (olpefit_amd/covariance.py).
 * The pivot: given at create, or set on the device by the first fold from its first row
 * (walker 0, row 0; a non-finite entry becomes 0.0); it then stays fixed until reset.  An
 * unlucky pivot costs precision, not correctness: the relative error of a variance read
 * from the sums grows as 1 + (mean - p)^2 / sigma^2.
 * No floating-point atomics: every sum runs in an order fixed by the fold's shape (per
 * workgroup partial sums over fixed runs of 256-row tiles, then one fixed tree), so the
 * same fold of the same rows gives the same bits whatever the device or grid.  The state is
 * additive over folds, objects, ranks and checkpoints whose pivots are bit-equal.  An
 * olpe_cov belongs to a device, not to a sampler context.  Calls on one object are not
 * thread-safe.  Not covered: per-walker covariance matrices, sky-frame ellipses, a
 * collective over the state. */
typedef struct olpe_cov olpe_cov;
/* The set-up of apf_step3.py:603-643's pair sums: 1 <= ncols <= 24; walkers 0 (pooled sums
 * only) or the ensemble's walker count, at most 65535 x 64; pivot [ncols], all finite, or
 * NULL (the first fold sets it).  Anything else is OLPE_EINVAL, naming the value, before
 * any GPU call; a per-walker store the device cannot hold is OLPE_ENOMEM naming its bytes.
 * OLPE_COV_TILE=64|128|256 sets the fold kernel's rows per tile (a test knob, 256 by
 * default: results agree to rounding, not to the bit, across tiles). */
int olpe_cov_create(int device, int ncols, long long walkers, const double *pivot,
                    olpe_cov **out);
/* Frees the object of apf_step3.py:603-643's pair sums (waits for its folds in flight). */
void olpe_cov_destroy(olpe_cov *h);
/* The sums (apf_step3.py:603-643's pairs) for rows 0, row_step, 2 row_step, ... of every
 * walker of ctx's last launch, read from its device chain in place (async on the context's
 * stream, no host copy; ncols == PS).  Once per launch: OLPE_ESTATE if this launch was
 * folded already; OLPE_EINVAL for row_step < 1, for a context of another device or PS, and,
 * with walkers > 0, of another walker count. */
int olpe_cov_fold_ctx(olpe_cov *h, olpe_ctx *ctx, int row_step);
/* The same sums (apf_step3.py:603-643's pairs) for host rows, walker-major
 * [nwalkers][nrows][ncols] (time_major 0) or time-major [nrows][nwalkers][ncols] (1, step
 * 3's chains), uploaded as they lie (no transposition) in pieces of at most 256 MiB.  With
 * walkers > 0 nwalkers must equal it; with walkers 0 the first two dimensions are just
 * rows.  A fold that fits one piece runs the kernels of olpe_cov_fold_ctx on the same
 * layout: a launch's chain read back and folded here gives that fold's bits. */
int olpe_cov_fold_rows(olpe_cov *h, const double *rows, long long nwalkers, long long nrows,
                       int time_major);
/* The pooled state so far (apf_step3.py:603-643's pairs summed): *n, *skipped, *has_pivot
 * (0 until a pivot is given or set), pivot [ncols] (zeros while there is none), S1 [ncols],
 * S2 [ncols][ncols]; any may be NULL.  Waits for the folds in flight. */
int olpe_cov_get(olpe_cov *h, unsigned long long *n, unsigned long long *skipped,
                 int *has_pivot, double *pivot, double *S1, double *S2);
/* The walkers' part of the state (apf_step3.py:169-205's chains, one per walker): nw
 * [walkers], S1w [walkers][ncols]; either may be NULL.  OLPE_ESTATE for an object created
 * with walkers 0.  Waits for the folds in flight. */
int olpe_cov_walkers_get(olpe_cov *h, unsigned long long *nw, double *S1w);
/* The between-walker term of the multivariate Gelman-Rubin statistic over
 * apf_step3.py:169-205's chains, reduced on the device in a fixed order: B [ncols][ncols]
 * = sum over the walkers with nw > 0 of S1w[w][j] S1w[w][k] / nw[w] (both triangles, bit-
 * equal), *m the number of such walkers, *nw_min and *nw_max the extremes of their counts (0
 * with no such walker); any may be NULL.  OLPE_ESTATE for an object created with walkers 0. */
int olpe_cov_between(olpe_cov *h, double *B, unsigned long long *m, unsigned long long *nw_min,
                     unsigned long long *nw_max);
/* Adds another object's, rank's or checkpoint's state (apf_step3.py:603-643's pairs over
 * the union of their rows); nw and S1w are read with walkers > 0 only.  OLPE_EINVAL, naming
 * which differs, if its ncols, its walkers or any bit of its pivot differ (the state is then
 * untouched); an object without a pivot yet adopts the incoming one. */
int olpe_cov_add(olpe_cov *h, int ncols, long long walkers, unsigned long long n,
                 unsigned long long skipped, const double *pivot, const double *S1,
                 const double *S2, const unsigned long long *nw, const double *S1w);
/* Zeroes the state (apf_step3.py:603-643 starts over); a pivot given at create stays, an
 * automatic one is forgotten; the launch folded last may be folded again. */
int olpe_cov_reset(olpe_cov *h);

/* --- companion detection map (apf_step2.py:78-124, :134-137) -----------------------------
 * "Is there another source in this frame, and how faint a one would have been seen?"  At
 * every candidate position c = (x_c, y_c) of the lattice x_c, y_c = j / oversample, j = 0 ..
 * oversample (n - 1) (G = (oversample (n - 1) + 1)^2 candidates, row y_c major), the
 * matched filter of a sample's residual with that sample's own unit PSF: with theta the
 * sample, M its build_analytical_model (EXACT operation order, whatever the context's eval
 * mode), err as apf_step2.py:210 (the 1 / err the context staged), pixels i,
 *   psi(u, v) = (1 - q) g1(u, v) + q g2(u - dx, v - dy)          (apf_step2.py:78-103)
 *   g_k(u, v) = exp(-((a_k u^2) + (b_k u) v + c_k v^2))          (narrow k = 1, wide k = 2)
 *   z_i = w_i (D_i - M_i),  w_i = (1 / err_i)^2, 0 where masked,  K_i = psi(x_i - x_c, y_i - y_c)
 *   N = sum_i z_i K_i,  Q = sum_i w_i K_i^2,  A = N / Q,  sigma_A = 1 / sqrt(Q),  snr = N / sqrt(Q)
 * A is the maximum-likelihood amplitude of one more source of the shared shape, in the units
 * of A_k - b.  It is a score test: the fitted sources stay at the sample's values, nothing
 * is refitted, and near a fitted source A is degenerate with that source's amplitude.  A
 * candidate no unmasked pixel sees (Q = 0) is NaN in every plane.  Folded over the samples
 * are five planes [G] of sums shifted about the pivot vector's planes: sum (A - A_p),
 * sum (A - A_p)^2, sum sigma_A^2, sum (snr - snr_p), sum (snr - snr_p)^2.  Counts, pivot,
 * best row, unusable rows and additivity follow olpe_resid's rules.  No floating-point
 * atomics: a candidate's sums take the same additions in the same order on any grid or CU
 * count.  Calls on one object are not thread-safe.  Not covered: refitting with the extra
 * source, a factorised (FAST) fold, a collective over the state. */
typedef struct olpe_detect olpe_detect;
#define OLPE_DETECT_SUMS 5
#define OLPE_DETECT_PLANES 10
/* olpe_detect_finalize's planes [OLPE_DETECT_PLANES][G], over the folded samples:
 *   [0] mean of A        [1] its np.std (ddof 0)      [2] sqrt(mean sigma_A^2)
 *   [3] sqrt(mean sigma_A^2 + var A): the law of total variance, the PSF posterior's scatter
 *       counted                                        [4] mean of snr      [5] its std
 *   [6] [0] / [3]        [7] A, [8] sigma_A, [9] snr of the best sample.  Its scalars: */
#define OLPE_DETECT_SCALARS 8
#define OLPE_DETECT_USED 0      /* samples folded (usable) */
#define OLPE_DETECT_BAD 1       /* unusable rows met */
#define OLPE_DETECT_PIXELS 2    /* unmasked pixels */
#define OLPE_DETECT_BLIND 3     /* candidates with Q = 0 */
#define OLPE_DETECT_MAX6 4      /* max of plane 6 ... */
#define OLPE_DETECT_MAX6_AT 5   /* ... and its candidate (the lowest on a tie; -1: none) */
#define OLPE_DETECT_MIN6 6      /* min of plane 6 */
#define OLPE_DETECT_MED3 7      /* median of plane 3 over the candidates that are not NaN */
/* Copies ctx's staged cutout (apf_step2.py:176-210: data, 1/err, mask) device to device and
 * takes its side, sources, bkgd_mode and device; independent of ctx afterwards.  pivot: a
 * parameter vector (its PS - 1 parameters are read, all finite), or NULL: the first usable
 * row folded becomes the pivot.  OLPE_EINVAL for an oversample outside {1, 2, 4} and for a
 * side above 128. */
int olpe_detect_create(olpe_ctx *ctx, const double *pivot, int oversample, olpe_detect **out);
/* Frees the object of apf_step2.py:78-124's map (waits for its folds in flight). */
void olpe_detect_destroy(olpe_detect *d);
/* The map of apf_step2.py:78-124 for rows 0, row_step, ... of walkers 0, walker_step, ... of
 * ctx's last launch, read from its device chain in place, walker-major (async on the
 * context's stream, no copy).  Once per launch: OLPE_ESTATE if this launch was folded
 * already; OLPE_EINVAL for a context of another device, side, nsrc or bkgd_mode. */
int olpe_detect_fold_ctx(olpe_detect *d, olpe_ctx *ctx, int row_step, int walker_step);
/* The map of apf_step2.py:78-124 for host rows [nsamples][PS], uploaded in bounded pieces. */
int olpe_detect_fold_rows(olpe_detect *d, const double *rows, long long nsamples);
/* The state (apf_step2.py:78-124 summed): samples used, unusable rows, pivot [PS], the sums
 * [OLPE_DETECT_SUMS][G], best row [PS]; any may be NULL; pivot / best are NaN while there is
 * none.  Waits for the folds in flight. */
int olpe_detect_get(olpe_detect *d, long long *n, long long *n_bad, double *pivot, double *sums,
                    double *best);
/* Adds another object's, rank's or checkpoint's state (apf_step2.py:78-124 over the union of
 * their rows).  OLPE_EINVAL if the pivots' parameters differ in any bit, unless this object
 * holds no sample yet: it then adopts the incoming pivot.  This object's rows count as
 * folded first: the incoming best row wins only with a strictly smaller chi^2. */
int olpe_detect_add(olpe_detect *d, long long n, long long n_bad, const double *pivot,
                    const double *sums, const double *best);
/* Empties the state (apf_step2.py:78-124 starts over); a pivot given at create stays. */
int olpe_detect_reset(olpe_detect *d);
/* A, sigma_A and snr [3][G] of one explicit vector (apf_step2.py:78-124 at its PS - 1
 * parameters, all finite); the state is left as it is. */
int olpe_detect_point(olpe_detect *d, const double *vec, double *planes);
/* The planes and scalars above (apf_step2.py:78-137 per plane) from the state, which it
 * leaves as it is: more folds and another finalize may follow.  OLPE_ESTATE with no usable
 * sample, or when no usable sample's chi^2 is a number. */
int olpe_detect_finalize(olpe_detect *d, double *planes, double *scalars);

/* --- false-alarm calibration of the detection map (apf_step2.py:78-124, :210) -------------
 * "What does a 5 sigma candidate of this map mean?"  A candidate's snr is standard normal
 * under the noise model, a map is up to 259,081 strongly correlated candidates: what counts is
 * the distribution of the map's maximum with no further source in the frame.  theta is one
 * parameter vector; K_i(c), w_i, Q(c) are the map's at theta.  Realisation r, r = 0, 1, ...:
 *   eps_r = np.random.RandomState((seed + r) mod 2^32).standard_normal(n n) in raster order
 *           (MT19937, the legacy polar method); every pixel takes a draw, masked or not
 *   y_r,i = eps_r,i (1 / err_i), 0 at masked pixels (the 1 / err the context staged)
 *   snr_r(c) = scale(c) ((sum_i K_i(c) y_r,i) / sqrt(Q(c))), NaN where Q(c) = 0
 * Each map is reduced on the device; NaN candidates are left out everywhere:
 *   max_all, argmax_all  the maximum and its candidate (row * g + column; the first on a tie;
 *                        NaN and -1 with no candidate)
 *   max_out, argmax_out  the same over the candidates farther than exclude_px from every
 *                        known source (detect.py's flag)
 *   peaks_all, peaks_out the strict local maxima at or above the threshold over the 8 lattice
 *                        neighbours, a NaN neighbour counting as none (a plateau has none)
 *   ring_max [nring]     the maximum of ring k = floor(hypot(x - cx, y - cy) / bin_px), NaN
 *                        for a ring without a candidate; nring = the largest ring + 1
 * The order of a candidate's additions depends on the frame's shape only, never on the batch
 * size, the number of realisations or the position in a batch; no floating-point atomics.
 * The fit is not redone per realisation.  Calls on one object are not thread-safe. */
typedef struct olpe_detect_null olpe_detect_null;
/* Evaluates d at vec (its PS - 1 parameters, all finite) and copies the tables, Q and the
 * staged cutout (apf_step2.py:78-103, :210): independent of d afterwards.  scale [G] finite
 * and > 0, or NULL for 1; known [nknown][2] the fitted sources' (x, y); centre [2];
 * batch: realisations per batch, 0 = from a byte budget (any value gives the same bits).
 * Arguments are checked before any GPU call. */
int olpe_detect_null_create(olpe_detect *d, const double *vec, const double *scale,
                            const double *known, int nknown, double exclude_px,
                            const double *centre, double bin_px, double threshold,
                            unsigned long long seed, int batch, olpe_detect_null **out);
/* Frees the object of apf_step2.py:78-124's null maps. */
void olpe_detect_null_destroy(olpe_detect_null *h);
/* count more realisations of apf_step2.py:78-124's map under the noise of :210, generated
 * on the device, continuing at realisation index `done`.  OLPE_ESTATE after
 * olpe_detect_null_run_frames on the same object. */
int olpe_detect_null_run(olpe_detect_null *h, long long count);
/* count realisations of apf_step2.py:78-124's map from explicit host noise eps
 * [count][n][n] in place of the generator.  OLPE_ESTATE after olpe_detect_null_run. */
int olpe_detect_null_run_frames(olpe_detect_null *h, const double *eps, long long count);
/* The reductions of apf_step2.py:78-124's null maps, per realisation so far: *done, *nring,
 * then arrays [done] (ring_max [done][nring]); any may be NULL. */
int olpe_detect_null_get(olpe_detect_null *h, long long *done, int *nring, double *max_all,
                         long long *argmax_all, double *max_out, long long *argmax_out,
                         long long *peaks_all, long long *peaks_out, double *ring_max);
/* Recomputes apf_step2.py:78-124's snr maps [count][G] of the generated realisations r0 ..
 * r0 + count - 1; the results so far are left as they are. */
int olpe_detect_null_maps(olpe_detect_null *h, long long r0, long long count, double *out);
/* The noise frames eps [count][n][n] (apf_step2.py:210's unit deviates) of the generated
 * realisations r0 .. r0 + count - 1. */
int olpe_detect_null_noise(olpe_detect_null *h, long long r0, long long count, double *out);
/* Forgets the realisations (apf_step2.py:78-124 starts over at index 0, generated or
 * explicit). */
int olpe_detect_null_reset(olpe_detect_null *h);

#ifdef __cplusplus
}
#endif
#endif /* OLPE_H */
