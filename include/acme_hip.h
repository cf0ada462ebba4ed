/* acme_hip.h -- C ABI of libacme_hip.so: batched, MI355X-native run!(::DiscreteModel, u).
 *
 * This is the drop-in boundary for the one hot path of ACME.jl that this project
 * accelerates.  Everything is plain C: pointers, sizes, integer status codes; no C++
 * or torch types.  A maintainer binds it from Julia with `ccall` (see INTEGRATION.md for
 * the glue that implements ModelRunner/run! on top of it); this repository's own host
 * side binds it from Python with ctypes (acme_jl_amd/runner.py).
 *
 * Reference interfaces replaced (file:line relative to the ACME.jl tree):
 *   DiscreteModel data .............................. src/ACME.jl:118-148
 *   closures func/set_p/calc_Jp -> element table .... src/ACME.jl:176-194,236-252,
 *                                                     src/circuit.jl:6-20,68-86
 *   ModelRunner(model, showprogress) ................ src/ACME.jl:570-604
 *   run!(runner, y, u) / step! ...................... src/ACME.jl:650-715
 *   solver plugin contract (set_resabstol!, get/set_extrapolation_origin,
 *     hasconverged, needediterations) ............... src/solvers.jl:181-205,262-302
 *
 * Conventions
 *   * All matrices are column-major Float64, exactly Julia's Matrix{Float64} layout.
 *   * A batch holds N independent instances of one model.  u is [N][T][nu] and y is
 *     [N][T][ny] doubles, i.e. instance i's block is the reference's nu x T (ny x T)
 *     column-major matrix, blocks back to back; a batch of one is bit-layout identical
 *     to the reference's u and y.
 *   * Every entry point returns ACME_OK (0) or a negative error code and never unwinds;
 *     acme_last_error() returns a thread-local message for the last failure.
 *   * Threading: handles are single-owner; distinct handles are independent.
 *   * Devices: a batch lives on one HIP device (acme_options.device); every entry point switches
 *     to it for the duration of the call and restores the caller's current device on return.
 *   * Failure semantics of step! (src/ACME.jl:688-694) are reported per instance in
 *     acme_report: n_warn counts "Failed to converge" warnings; first_nonfinite >= 0 is
 *     the sample at which the reference would have thrown -- that instance stops
 *     advancing there (its x stays at that sample, y from there on is NaN).
 */
#ifndef ACME_HIP_H
#define ACME_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define ACME_OK 0
#define ACME_ERR_INVALID (-1)     /* bad argument / DimensionMismatch */
#define ACME_ERR_UNSUPPORTED (-2) /* model does not fit the kernel (see message) */
#define ACME_ERR_HIP (-3)         /* HIP runtime failure */
#define ACME_ERR_NO_DEVICE (-4)   /* no usable GPU: the product path has no CPU fallback */

/* element kinds of the nonlinear element table and their parameter vectors
 * (ACME_MAX_ELEM_PAR doubles per element, unused entries zero) */
#define ACME_KIND_DIODE 1  /* is, eta                                   src/elements.jl:236-245 */
#define ACME_KIND_BJT 2    /* ise,isc,etae,etac,bf,br,ile,ilc,etael,etacl,vaf,var,ikf,ikr
                                                                       src/elements.jl:309-406 */
#define ACME_KIND_POT 3    /* r                                         src/elements.jl:20-31   */
#define ACME_KIND_MOSFET 4 /* polarity,lambda,nvt,vt[4],nalpha,alpha[4] src/elements.jl:436-481
                              (the reference takes polynomials of any length, :436-450; here 1 ... 4 coefficients
                              each: acme_model_add_subproblem returns ACME_ERR_UNSUPPORTED beyond that) */
#define ACME_KIND_MACAK 5  /* gain, scale                               src/elements.jl:536-551 */
#define ACME_KIND_JA 6     /* Ms,a,alpha,c,k                            src/elements.jl:100-135 */
#define ACME_MAX_ELEM_PAR 16

/* solver selection = third positional argument of DiscreteModel (src/ACME.jl:150) */
#define ACME_SOLVER_SIMPLE 0   /* SimpleSolver                  src/solvers.jl:151-236 */
#define ACME_SOLVER_HOMOTOPY 1 /* HomotopySolver{SimpleSolver}  src/solvers.jl:247-302 */
/* HomotopySolver{CachingSolver{SimpleSolver}} (src/solvers.jl:303-405, the reference's default
 * stack) with a BOUNDED store: per instance and sub-problem the last 16 stored solutions, first in
 * first out, instead of the reference's ever-growing k-d tree.  Same lookup rule (a stored p
 * strictly nearer than the current extrapolation origin becomes the origin) and storing rule
 * (converged base solve that needed more than 5 iterations). */
#define ACME_SOLVER_CACHING_HOMOTOPY 2

/* where u / y live */
#define ACME_MEM_HOST 0
#define ACME_MEM_DEVICE 1

typedef struct acme_model acme_model;
typedef struct acme_batch acme_batch;

typedef struct {
    int solver;    /* ACME_SOLVER_*; default HOMOTOPY */
    double tol;    /* residual max-abs tolerance, default 1e-10 (src/solvers.jl:175) */
    int maxiter;   /* Newton iterations per base solve, default 500 (src/solvers.jl:207) */
    int device;    /* HIP device ordinal, -1 = current device */
    int per_instance_matrices; /* 0: all instances share the model's matrices;
                                  1: every instance has its own (acme_batch_set_matrices) */
} acme_options;

typedef struct {
    long long n_warn;             /* "Failed to converge" warnings so far            */
    long long first_nonconverged; /* 0-based sample of the first warning, -1 if none */
    long long first_nonfinite;    /* 0-based sample of the fatal error, -1 if none   */
    long long iters_total;        /* sum of needediterations over all samples        */
    long long iters_max;          /* max needediterations of one sample              */
} acme_report;

const char *acme_last_error(void);
/* number of visible HIP devices (0 if none / runtime unavailable) */
int acme_device_count(void);
void acme_default_options(acme_options *opts);

/* ---- model: the data of struct DiscreteModel (src/ACME.jl:118-148) ------------------ */
int acme_model_create(int nx, int nu, int ny, int nn_total, const double *a, const double *b,
                      const double *c, const double *x0, const double *dy, const double *ey,
                      const double *fy, const double *y0, acme_model **out);
/* one nonlinear sub-problem: pexps/dqs/eqs/fqprevs/fqs/q0s[idx] (src/ACME.jl:123-128), the
 * initial extrapolation origin z (p = 0; src/ACME.jl:253-259) and the element table in
 * CircuitNLFunc order (src/circuit.jl:68-86); elem_par is n_elems x ACME_MAX_ELEM_PAR
 * row-major */
int acme_model_add_subproblem(acme_model *m, int nn, int nq, int np, const double *pexp,
                              const double *dq, const double *eq, const double *fqprev,
                              const double *fq, const double *q0, const double *init_z,
                              int n_elems, const int *elem_kind, const int *elem_qoff,
                              const int *elem_roff, const double *elem_par);
/* optional performance hint: order[pos] = residual row (0-based, in element-table order)
 * handled by lane `pos` when a batch is created.  The elimination keeps the row sitting in pivot
 * position while every multiplier satisfies |l| <= 8 (threshold partial pivoting; the
 * reference's setlhs!, src/solvers.jl:58-78, is the threshold 1) and only otherwise re-learns
 * the order with the reference's first-strict-maximum search; listing the equations in their
 * usual pivot order spares the first such searches.  Either way the factorisation is a valid LU
 * of the same Jacobian: results of different row orders agree to rounding.  n = 0 restores the
 * natural order. */
int acme_model_set_row_order(acme_model *m, int sub, const int *order, int n);
void acme_model_destroy(acme_model *m);
/* dims = {nn, nq, np, nx, nu, ny} of the instantiated kernel shape the model runs in */
int acme_model_kernel_shape(const acme_model *m, int dims[6]);
/* which kernel variant the model runs in: *condensed_rows = number of residual rows eliminated ahead of
 * the Newton iteration (the potentiometer rows of DESIGN.md 2 "Round 4"; 0 = none), *generic = 0 for a tuned
 * shape; 2 when no instantiated shape holds the model and the cooperative run-time-sized kernel takes it (one
 * sub-problem of up to 64 unknowns, working arrays in LDS: csrc/acme_coop.h); 1 for the lane-per-instance kernel
 * that takes everything else (csrc/acme_generic.h).  Either pointer may be null. */
int acme_model_kernel_variant(const acme_model *m, int *condensed_rows, int *generic);

/* ---- batch: N instances + their device-resident mutable state ----------------------- */
/* state starts like a fresh DiscreteModel: x = 0 (src/ACME.jl:145), origin (0, init_z) */
int acme_batch_create(const acme_model *m, long long n_instances, const acme_options *opts,
                      acme_batch **out);
void acme_batch_destroy(acme_batch *b);
/* which kernel variant THIS BATCH runs in, as acme_model_kernel_variant reports it for a model (*family: 0 tuned shape, 1
 * lane-per-instance generic kernel, 2 cooperative mid-size kernel).  It can differ from its model's: instances with element
 * parameters of their own (acme_batch_set_matrices) move a batch off the condensed shape (the library rebuilds it on the
 * plain shape by itself: the reference's models each carry their own closures, src/elements.jl:236-245,309-406) and a
 * mid-size batch to the lane-per-instance kernel.  Either pointer may be null. */
int acme_batch_kernel_variant(const acme_batch *b, int *condensed_rows, int *family);

/* per-instance matrices (Monte-Carlo component tolerances, sweeps over element parameters): instance i uses the
 * matrices AND the element closures' parameters of models[i] -- in the reference every model carries its own element
 * closures (src/elements.jl:236-245, 309-406).  All models must have the batch model's dimensions and circuit
 * STRUCTURE (the same element kinds in the same residual rows reading the same q entries); the element parameters
 * -- a diode's is / eta, a transistor's betas, which Gummel-Poon refinements it has -- may differ: the batch then
 * keeps one element table per instance (a block of the 16-lane kernels stages its 16 tables in LDS; if they do not
 * fit a compute unit the call fails with ACME_ERR_UNSUPPORTED).  The instances take the freshly constructed state of their model (x = 0, each
 * solver's extrapolation origin at p = 0, z = the model's init_z; src/ACME.jl:145,253-259).
 * Only valid for batches created with per_instance_matrices = 1. */
int acme_batch_set_matrices(acme_batch *b, long long first, long long count,
                            const acme_model *const *models);

/* run!(runner, y, u): advance every instance by T samples (src/ACME.jl:650-664).
 * mem = ACME_MEM_HOST: u/y are host buffers, copied in time slices that overlap the kernel.  On a batch with
 *   acme_batch_set_host_retention (arrays page-locked and mapped), runs of 4096+ samples are STREAMED: one launch;
 *   the kernel writes y to the caller's array itself and reads u from an HBM staging buffer the copy engine fills
 *   while the kernel runs (waves that get ahead of the copy wait) -- the device-resident rate; not with a progress
 *   callback installed, for memory that cannot be page-locked, for batches of more blocks than the chip holds at
 *   once, nor for the lane-per-instance and generic kernels (time slices).  The call returns when y is complete;
 * mem = ACME_MEM_DEVICE: u/y are device pointers on the batch's device and `stream` is the
 * hipStream_t to launch on (NULL = default stream); the call is then asynchronous.
 * y = NULL is accepted (here, by acme_batch_run_const and by acme_batch_run_async) only while a measurement is armed
 * (acme_batch_set_measurement, below). */
int acme_batch_run(acme_batch *b, const double *u, double *y, long long T, int mem,
                   void *stream);
/* run! with CONSTANT input rows (src/ACME.jl:672-674 copies column n of u into ucur sample by sample: a row that never
 * changes -- a potentiometer position, a supply voltage, a mix control of a parameter sweep -- need not be materialised
 * T times).  const_mask: bit k set = input row k keeps the value u_const[i * nu + k] (u_const: [N][nu], the entries of
 * the other rows are ignored) for the whole call; u_var then holds only the rows whose bit is clear, in row order:
 * [N][T][nu_var] with nu_var = nu - popcount(const_mask).  The full input rows are put together ON THE DEVICE, time
 * slice by time slice (HBM traffic the kernels do not notice), so a host-buffer run moves nu_var / nu of the bytes
 * over the bus -- the headline sweep (three pot rows of four inputs): 2.9 instead of 11.6 GB per second of audio.
 * Results are those of acme_batch_run on the materialised u, bit for bit.  mem / stream as acme_batch_run (u_var and
 * u_const live where mem says); y: [N][T][ny].  Host arrays: time slices copied in and out beside the kernels; with
 * acme_batch_set_host_retention u_var and y are page-locked once and kept (headline: 0.92 x the device-resident rate). */
int acme_batch_run_const(acme_batch *b, const double *u_var, const double *u_const, unsigned long long const_mask,
                         double *y, long long T, int mem, void *stream);
/* Host-buffer runs and page-locking.  By DEFAULT the library never keeps anything of the caller's arrays beyond the
 * call: u and y are copied from / to ordinary (pageable) memory in time slices that overlap the kernel -- the right
 * thing for one-shot calls and for wrappers whose arrays are per-call temporaries or garbage-collected (locking
 * 14.4 GB costs more than running them: headline 0.39 s this way, 0.70 s locked and streamed).
 * keep != 0: the caller PROMISES that the arrays it passes stay allocated until it passes others, calls
 * acme_batch_release_host_buffers or destroys the batch.  The library then page-locks and maps them
 * (hipHostRegister) on first use and keeps the last range of each direction locked: runs of 4096+ samples are
 * STREAMED (see acme_batch_run) at the device-resident rate -- what the in-place run!(runner, y, u) with reused
 * arrays is for (src/ACME.jl:650-664).  Memory that cannot be locked is copied from as it is.
 * ACME_HOST_REGISTER=0 in the environment disables the locking altogether. */
int acme_batch_set_host_retention(acme_batch *b, int keep);
/* un-page-lock what a retaining batch (above) holds: before the caller frees or resizes its arrays while the
 * batch lives on.  Idempotent. */
int acme_batch_release_host_buffers(acme_batch *b);
/* @showprogress of run!(runner, y, u) (src/ACME.jl:587-604,653): `fn(user, samples_done, samples_total)`
 * is called on the calling thread (the worker thread of an asynchronous run) after every time slice of a
 * host-buffer run -- 8 to 24 per run of 4096+ samples; a callback makes such a run sliced rather than streamed,
 * at ~0.91 of the speed -- and once at the end of any other run.  fn = NULL removes it.  The callback must not
 * call into the batch. */
typedef void (*acme_progress_fn)(void *user, long long samples_done, long long samples_total);
int acme_batch_set_progress_callback(acme_batch *b, acme_progress_fn fn, void *user);

/* Oversampled runs.  A nonlinear model run at the audio rate fs aliases its own harmonics back into the audio band, so
 * models are derived at k fs.  A batch with a factor k (1 ... ACME_MAX_OVERSAMPLING) takes u [N][T][nu] and returns
 * y [N][T][ny] at the BASE rate fs through every run entry point (acme_batch_run, _run_const, _run_async; host and device
 * memory) while its model -- the caller's DiscreteModel, derived at k fs -- advances k T samples:
 *   interpolation  for each input row that is not held: s[m] = u[m/k] if k divides m, else 0;
 *                  u_os[m] = sum_{j=0}^{Lu-1} g[j] s[m-j]  with g = k h_up (the library multiplies by k once, on the host)
 *   held rows      u_os[m] = u[floor(m/k)] (zero-order hold): the rows of the mask held_rows -- pot positions, supplies, mix
 *                  controls -- and the constant rows of acme_batch_run_const, always
 *   decimation     y[n] = sum_{j=0}^{Ld-1} h_down[j] y_os[n k + k - 1 - j]
 * Every sum runs over ascending j as a chain of fma: results are bit-identical across host and device memory, time slices
 * and split calls.  Before the first run after the factor is set, each signal extends its first value into the past
 * (u[n < 0] = u[0], y_os[m < 0] = y_os[0]: a DC input, or an instance set to its steady state, starts without a filter
 * transient); from then on the histories are carried from call to call (T1 then T2 samples = one run of T1 + T2, bit for
 * bit).  acme_batch_set_matrices zeroes the histories of the instances it makes afresh; acme_batch_set_state leaves them
 * alone.  COUNTERS: acme_report counts model-rate samples (first_nonconverged / first_nonfinite are model-rate indices,
 * k n + phase); the progress callback counts base-rate samples.
 * Runs go slice by slice on the launch stream (interpolate, the unchanged run kernel over k x the slice, decimate; bounded
 * scratch); host buffers take the sliced copy pipeline, never the streamed path of acme_batch_set_host_retention.  Not
 * together with acme_batch_set_isolation (ACME_ERR_UNSUPPORTED either way round). */
#define ACME_MAX_OVERSAMPLING 16
/* the library's default lowpass for `factor`: a linear-phase Kaiser-windowed sinc at the high rate, unit DC gain, passband
 * to 0.40 fs (ripple below 1e-4), at least 80 dB from 0.50 fs; length L odd and L = 1 (mod factor), so the pair delays the
 * signal by the whole number (L - 1) / factor of base-rate samples.  Returns L (or a negative error code) and writes the taps
 * when capacity >= L.  Factor 1: the single tap 1. */
int acme_oversampling_design(int factor, double *taps, int capacity);
/* set the batch's factor (1 switches oversampling off: today's path, none of the resampling runs) and filters: h_up /
 * h_down with n_up / n_down (1 ... 4096) taps, NULL = the default design; held_rows bit r = input row r held.  Validates
 * its arguments (ACME_ERR_INVALID) and resets the histories. */
int acme_batch_set_oversampling(acme_batch *b, int factor, const double *h_up, int n_up, const double *h_down, int n_down,
                                unsigned long long held_rows);

/* Output measurements.  What a sweep usually wants back is a few numbers per cell -- DC offset, RMS, peak, the gain at the
 * fundamental, the harmonic distortion (SPICE's .four / .meas) --, not all of y.  While a measurement is armed, every run
 * entry point (acme_batch_run, _run_const, _run_async; host and device memory; oversampled batches: the base-rate y, after
 * decimation) feeds the library's accumulators on the device, and y may be NULL: nothing of it is then written, staged or
 * copied back (the device needs one time slice of output scratch, not [N][T][ny]).
 *   window      samples are counted from arming (acme_batch_set_measurement / _reset_measurement) across every later run;
 *               sample n counts when start <= n < start + length (length 0: every sample from start on); m = n - start
 *   per instance and measured row, each accumulator ONE chain in sample order:
 *               sum += y;  sq = fma(y, y, sq);  min;  max;
 *               C_h = fma(y, cos th, C_h),  S_h = fma(y, sin th, S_h)  for h = 1 ... H,
 *               th = 2 pi ((h f_num m) mod f_den) / f_den  (the phase reduced exactly in 64-bit integers)
 *   results     acme_batch_get_measurement writes out[N][nrows][4 + 2H]: mean = sum / count, RMS = sqrt(sq / count), min,
 *               max, then Re and Im of A_h = (2 / count) (C_h - j S_h) for h = 1 ... H -- the complex amplitude of the h-th
 *               harmonic (y = |A_h| cos(h w n + arg A_h) gives A_h over whole periods); rows ascending; count = samples
 *               measured (0: NaN means).
 * Results do not depend on time slices, host or device memory, the entry point, split calls or whether y is stored (bit for
 * bit).  An instance past its first_nonfinite sample (NaN outputs) measures NaN; the others are unaffected.  While a
 * measurement is armed, host-buffer runs take the staged slice pipeline, never the streamed path of
 * acme_batch_set_host_retention.  acme_batch_set_matrices, _set_state, _reset_report and _set_oversampling leave the
 * accumulators and the window's position alone.  Not together with acme_batch_set_isolation (ACME_ERR_UNSUPPORTED either way
 * round).  Nothing armed: no launch, allocation or synchronisation of any run changes. */
#define ACME_MAX_HARMONICS 32
/* arm a measurement (zeroed accumulators, the window's clock at 0):
 *   start, length   first measured sample, counted in base-rate samples from arming; number of measured samples (0 = every
 *                   sample from start on)
 *   f_num, f_den    fundamental = f_num / f_den x the base sample rate (0 < f_den < 2^31)
 *   harmonics       H = 0 ... ACME_MAX_HARMONICS harmonics of the fundamental
 *   rows            output rows measured, bit r = row r; 0 = all rows (ny <= 64)
 * Validates its arguments (ACME_ERR_INVALID).  Completes the batch's outstanding work first.  (The window's parameters go
 * as plain arguments, not as a struct: a binding needs no mirror of the layout.) */
int acme_batch_set_measurement(acme_batch *b, long long start, long long length, long long f_num, long long f_den,
                               int harmonics, unsigned long long rows);
/* arm a measurement with a fundamental PER INSTANCE: the semantics of acme_batch_set_measurement with f_num replaced by
 * f_num[i] for instance i -- a frequency sweep driven by a per-instance sine source (below) is MEASURED in the same batch: a
 * Bode plot, THD against frequency, a drive x frequency grid, without [N][T][ny] anywhere.
 *   f_den, f_num    fundamental of instance i = f_num[i] / f_den x the base sample rate; f_num: a HOST array of N entries,
 *                   0 <= f_num[i] < f_den < 2^31, copied by the call (only read)
 * The formulas are the ones above with f_num -> f_num[i]: th = 2 pi (((h f_num[i]) mod f_den (m mod f_den)) mod f_den) / f_den,
 * the same cos / sin of the same angle, each accumulator ONE chain in sample order.  With every f_num[i] = f the results
 * are, bit for bit, those of acme_batch_set_measurement(f, f_den); instance i's results are, bit for bit, those of the
 * shared form at f_num[i].  acme_batch_get_measurement (out[N][nrows][4 + 2H], unchanged), _reset_measurement (the
 * frequencies stay) and _clear_measurement work as on any measurement; arming either form replaces the other;
 * acme_batch_set_matrices carries the frequencies with the accumulators.  Validates as the shared form does
 * (ACME_ERR_INVALID; an f_num[i] out of range is named by its instance); not together with acme_batch_set_isolation.
 * WHICH WINDOW: length = f_den samples hold whole periods of EVERY instance's fundamental (instance i: f_num[i] of them), and
 * so does every multiple of f_den / gcd(f_den, f_num[0], ..., f_num[N - 1]): that is the window of a sweep, after a start
 * that lets the transient die.
 * The instances are grouped by distinct f_num (csrc/acme_measure.h); a step's twiddle table takes at most 64 MiB, or one
 * tile of 64 samples per group and harmonic where that is more.  Test hook: ACME_MEAS_TABLE_BUDGET=bytes in the environment
 * at arming replaces the 64 MiB (results do not depend on it). */
int acme_batch_set_measurement_per_instance(acme_batch *b, long long start, long long length, long long f_den,
                                            long long *f_num /* host, [N], only read */, int harmonics,
                                            unsigned long long rows);
/* the plan of the armed per-instance or bins measurement (tests, probes; any pointer may be NULL): *n_groups distinct f_num, *chunk
 * samples per step (bins: *n_groups distinct tone tuples), perm[N nrows]: lane slot -> pair (i nrows + j), wave_group[(N nrows + 63) / 64]: the one group of the 64
 * slots' wave (the broadcast loop), or -1 (mixed: per-lane loads).  ACME_ERR_INVALID while no such measurement is armed. */
int acme_batch_get_measurement_plan(acme_batch *b, long long *n_groups, long long *chunk, long long *perm, int *wave_group);
/* arm a measurement whose BINS are integer combinations of per-instance tones: an intermodulation test (CCIF / DFD: 19 kHz +
 * 20 kHz read at f2 - f1, 2 f1 - f2, 2 f2 - f1; SMPTE: 60 Hz + 7 kHz read at f2 +- n f1) driven by a MULTISINE source (below) is
 * measured in the same batch.  The semantics of acme_batch_set_measurement with the harmonics h f_num replaced by the bins
 *   k[b][i] = (sum_j coef[b][j] f_num[j][i]) mod f_den    b = 0 ... bins - 1, the non-negative residue, exact 64-bit integers
 *   th = 2 pi ((k[b][i] (m mod f_den)) mod f_den) / f_den, C_b and S_b each ONE fma chain in sample order
 *   tones, f_num    1 ... ACME_MAX_SOURCE_TONES tones; f_num: a HOST array [tones][N] (tone j of instance i at f_num[j * N + i]),
 *                   0 <= f_num < f_den < 2^31, copied by the call (only read)
 *   bins, coef      0 ... ACME_MAX_HARMONICS bins; coef: a host array [bins][tones], |coef| <= 32767 (the sum stays below 2^48)
 * acme_batch_get_measurement writes out[N][nrows][4 + 2 bins]: the four moments (the same chains as ever), then Re and Im of
 * A_b = (2 / count) (C_b - j S_b).  Bin b of instance i is, bit for bit, harmonic 1 of acme_batch_set_measurement(f_num =
 * k[b][i], f_den, harmonics = 1) on an identical run; with tones = 1 and coef[b] = b + 1 the whole result is that of
 * acme_batch_set_measurement_per_instance with harmonics = bins.
 * NEGATIVE COMBINATIONS: a combination below zero is reduced into 0 ... f_den - 1 like any other: f2 - f1 with f1 > f2 becomes
 * f_den - (f1 - f2) -- the same spectral line of a real signal read at its mirror frequency, so |A_b| is the line's amplitude
 * and Im A_b comes out NEGATED (A_b is the conjugate of the amplitude at f1 - f2).  Choose the signs so that every bin is a
 * positive frequency (f1 - f2 here) when phases matter.  A bin with k = 0 reads C = the sum and S = 0 exactly.
 * The instances are grouped by distinct tone tuple (f_num[0][i], ...), in lexicographic order; plan, table budget, chunk rule,
 * ACME_MEAS_TABLE_BUDGET and acme_batch_get_measurement_plan are those of the per-instance form, and so are _reset_measurement
 * (the bins stay), _clear_measurement, acme_batch_set_matrices and the refusal with acme_batch_set_isolation.  Arming any of
 * the three forms replaces the others.  Validates as the per-instance form does (ACME_ERR_INVALID: tones or bins out of range,
 * null f_num, null coef with bins > 0, an f_num out of range -- named by tone and instance --, a coefficient out of range).
 * WHICH WINDOW: length = f_den samples hold whole periods of every tone and every product. */
int acme_batch_set_measurement_bins(acme_batch *b, long long start, long long length, long long f_den, int tones,
                                    long long *f_num /* host, [tones][N], only read */, int bins,
                                    const int *coef /* host, [bins][tones] */, unsigned long long rows);
/* A SERIES of windows: the armed measurement (any of the three forms, armed with length = 0, no sample fed since arming or
 * the last reset) measures `windows` windows of `win` samples, one every `hop` samples, all in the same pass over y -- a level
 * or a harmonic as a function of time: has the THD settled, a tone burst, the recovery after overload, a parameter stepped in
 * time with a settle gap (hop > win) between the readings.
 *   window w (0 <= w < windows) covers the samples start + w hop <= n < start + w hop + win, 1 <= win <= hop; the samples of a
 *   gap and those behind the last window belong to no window.
 * Window w holds, BIT FOR BIT, what the same form armed with start' = start + w hop, length' = win accumulates on an identical
 * run: the twiddle's phase is window-relative (m' = n - start - w hop), every accumulator one chain in sample order from its
 * start value.  Nothing depends on where chunks, slices or calls end, on the memory kind, the entry point, the oversampling
 * factor or on whether y is stored; a window the end of a run cuts is partial (its count the samples seen so far) and goes
 * on in the next call.  The accumulators take windows x (4 + 2H) x N nrows doubles of device memory.
 * ACME_ERR_INVALID (the message names the argument): no measurement armed, length != 0, samples already fed, win < 1,
 * hop < win, windows outside 1 ... ACME_MAX_SERIES_WINDOWS, start + (windows - 1) hop + win beyond 64 bits.  With a series
 * acme_batch_get_measurement is refused (ACME_ERR_INVALID, naming the getter below), _reset_measurement restarts every window
 * and the clock, arming any form or _clear_measurement removes the series, acme_batch_get_measurement_plan is unchanged and
 * acme_batch_set_matrices carries the series with the accumulators.  A batch without a series launches and allocates what
 * it always did. */
#define ACME_MAX_SERIES_WINDOWS 1048576
int acme_batch_set_measurement_series(acme_batch *b, long long win, long long hop, long long windows);
/* windows first ... first + n - 1 of the series: out[n][N][nrows][4 + 2H], each window in the format and scaling of
 * acme_batch_get_measurement (may be NULL); counts[n]: the samples measured so far per window (may be NULL).  A window never
 * reached has count 0 and reads NaN / +-inf as a fresh single window does.  ACME_ERR_INVALID without a series, or when
 * first + n exceeds the series' windows.  Joins a pending acme_batch_run_async and synchronises the device. */
int acme_batch_get_measurement_series(acme_batch *b, long long first, long long n, double *out, long long *counts);
/* A FOLD of the window onto one period (synchronous averaging): the armed measurement (any of the three forms, armed with any
 * start / length, no sample fed since arming or the last reset) also accumulates, per instance i with a period of P_i samples
 * (1 <= P_i <= ACME_MAX_FOLD_PERIOD), measured row j and slot s = m mod P_i of the window-relative sample number m = n - start,
 *   fold[i][j][s] += y        ONE chain per slot, plain additions in sample order, from 0.0
 * -- the periodic steady state's waveform itself, N x nrows x P doubles in place of y [N][T][ny]: the clipped wave across a
 * level sweep, a transfer curve, every harmonic up to Nyquist and the lines where aliasing lands (a host FFT of one period),
 * THD+N.  Sources and measurement windows run on exact rational frequencies f_num / f_den: the signal's period is the whole
 * number f_den / gcd(f_num, f_den) of samples (1 kHz at 44.1 kHz: 441).
 *   period, period_i   period_i = NULL: every instance folds onto `period`; otherwise a HOST array of N entries, instance i
 *                      folds onto period_i[i] and `period` is ignored (copied by the call, only read)
 * The fold depends on nothing but the run's samples: chunk, slice and call boundaries, host or device memory, the entry point
 * (acme_batch_run, _run_const, _run_async, _run_sources), the oversampling factor and whether y is stored change none of its
 * bits.  The measurement's own accumulators and launches are what they are without a fold; the fold takes one more kernel per
 * chunk of the window and N nrows max_i P_i doubles of device memory.
 * ACME_ERR_INVALID (the message names the argument, and the instance of an entry of period_i): no measurement armed, samples
 * already fed, a period outside 1 ... ACME_MAX_FOLD_PERIOD.  ACME_ERR_UNSUPPORTED together with a series, whichever is set
 * first: a fold per window is not available.  Setting a fold again replaces the earlier one.  _reset_measurement zeroes the fold
 * and keeps the periods, arming any form or _clear_measurement removes it, acme_batch_set_matrices carries it with the
 * accumulators; acme_batch_get_measurement and _get_measurement_plan are unchanged, and so is the refusal with
 * acme_batch_set_isolation.  A batch without a fold launches and allocates what it always did. */
#define ACME_MAX_FOLD_PERIOD 65536
int acme_batch_set_measurement_fold(acme_batch *b, long long period, long long *period_i /* host, [N] or NULL, only read */);
/* the fold so far: out[N][nrows][Pmax], Pmax = max_i P_i (may be NULL): out[i][j][s] = fold[i][j][s] / c_s, the mean of the
 * c_s = (count > s ? (count - s - 1) / P_i + 1 : 0) samples slot s has received; a slot nothing has reached, and every slot
 * s >= P_i, reads NaN, as the mean of an empty window does.  period[N]: the instances' periods (may be NULL); *count: samples
 * measured, as acme_batch_get_measurement counts them (may be NULL).  ACME_ERR_INVALID without a fold.  Joins a pending
 * acme_batch_run_async and synchronises the device. */
int acme_batch_get_measurement_fold(acme_batch *b, double *out, long long *period, long long *count);
/* the same slots undivided: out[N][nrows][Pmax] (not NULL), out[i][j][s] = fold[i][j][s], the chain's sum itself (the tests pin
 * it with ==; sums of separate runs can be added before dividing); the slots that read NaN above read NaN here. */
int acme_batch_get_measurement_fold_sums(acme_batch *b, double *out);
/* A SPECTRUM of the window (Welch's method): the armed measurement (any of the three forms, no sample fed since arming or the
 * last reset) also cuts its window [start, start + length) into overlapping segments of L samples, one every `hop` samples,
 * multiplies each by the window w, transforms it with an fp64 FFT on the device and accumulates |X_k|^2 over the segments, per
 * instance, measured row and bin k = 0 ... L / 2 -- the estimator for signals that are not periodic: the output of a
 * noise-driven run, THD+N, the noise floor between the harmonics, N x nrows x (L / 2 + 1) doubles in place of y [N][T][ny].
 *   L     a power of two, ACME_MIN_SPECTRUM <= L <= ACME_MAX_SPECTRUM
 *   hop   1 <= hop <= L
 *   w     HOST array of L finite values (copied by the call), or NULL: all 1.0
 * Segments: with m = n - start the window-relative sample number, segment s = 0, 1, ... covers m in [s hop, s hop + L).  It
 * contributes once all its samples have been fed and lie inside the window: after `count` samples
 * segments = count >= L ? (count - L) / hop + 1 : 0; samples beyond the last complete segment contribute nothing.
 * Arithmetic, per segment and pair -- every operation rounded on its own, NO fused multiply-add anywhere:
 *   1. x_j = w[j] y[s hop + j], one product; the imaginary part is 0.
 *   2. X = FFT_L(x), the radix-2 decimation-in-time transform: load in bit-reversed order; stages q = 1 ... log2 L with
 *      half-size h = 2^(q-1); a butterfly on a = v[i], b = v[i + h] with (wr, wi) = tw[(i mod h) (L / 2h)] computes
 *      tr = wr br - wi bi, ti = wr bi + wi br (two products and one subtraction / addition each) and stores v[i] = a + t,
 *      v[i + h] = a - t.
 *   3. for k = 0 ... L / 2: acc[k] += (Xr Xr + Xi Xi), ONE chain per bin in segment order from 0.0.
 * This fixes the VALUES, not the data flow (stages kept in registers, products with an exact 0.0 or 1.0 skipped and any
 * mapping to lanes give the same bits; signed zeros may differ).  tw[k] approximates (cos 2 pi k / L, -sin 2 pi k / L), k < L / 2,
 * made once at arming, each entry within 1.5 x 2^-53 of the exact value and exactly (1, 0) at k = 0, (0, -1) at k = L / 4.
 * The sums depend on nothing but the run's samples: chunk, slice and call boundaries, host or device memory, the entry point
 * (acme_batch_run, _run_const, _run_async, _run_sources, device pointers), y stored or NULL, the oversampling factor and
 * ACME_OS_SLICE change none of their bits.  The measurement's own accumulators and launches are what they are without a
 * spectrum; the spectrum takes one more kernel per chunk of the window and N nrows (L + L / 2 + 1) doubles of device memory
 * (the accumulators and a carry of the window's L most recent samples per pair).  A fold and a spectrum may be set together.
 * The kernel of a chunk transforms every segment that ends in the chunk, about chunk / hop per pair (a chunk is at most 4096
 * samples) in ONE launch: the cost grows as L log2 L / hop per sample, and a hop far below L / 8 on a wide batch makes that launch
 * long (hop = 1 at L = 4096 is 4096 transforms of 4096 points per pair and chunk).  Keep hop >= L / 8 on wide batches; smaller
 * hops are accepted and correct.
 * ACME_ERR_INVALID: no measurement armed, samples already fed, L not a power of two or out of range, hop out of range, a
 * non-finite window value.  ACME_ERR_UNSUPPORTED together with a series, whichever is set first.  Setting a spectrum again
 * replaces the earlier one.  _reset_measurement zeroes the sums and the carried samples and keeps L, hop, w and the table;
 * arming any form or _clear_measurement removes the spectrum; acme_batch_set_matrices carries it with the accumulators.  A
 * batch without a spectrum launches and allocates what it always did. */
#define ACME_MIN_SPECTRUM 64
#define ACME_MAX_SPECTRUM 4096
int acme_batch_set_measurement_spectrum(acme_batch *b, long long L, long long hop, const double *w /* host [L], NULL: all 1.0 */);
/* the spectrum so far: out[N][nrows][L / 2 + 1] (may be NULL) = acc / segments, NaN everywhere while segments == 0; *segments,
 * *count: complete segments and samples measured (may be NULL).  No scaling by the sample rate or the window's power is
 * applied.  ACME_ERR_INVALID without a spectrum.  Joins a pending acme_batch_run_async and synchronises the device. */
int acme_batch_get_measurement_spectrum(acme_batch *b, double *out, long long *segments, long long *count);
/* the same bins undivided: out[N][nrows][L / 2 + 1] (not NULL), the chains' sums themselves (NaN while segments == 0) */
int acme_batch_get_measurement_spectrum_sums(acme_batch *b, double *out);
/* the window w[L] and the table tw[L / 2][2] the kernel uses (either may be NULL) */
int acme_batch_get_measurement_spectrum_table(acme_batch *b, double *w, double *tw);
/* A CROSS-SPECTRUM of the window: the armed measurement (any of the three forms, no sample fed since arming or the last reset)
 * also relates ONE input row to every measured output row over the spectrum's segments -- Sxx, Syy and the complex Sxy per
 * instance, measured row and bin k = 0 ... L / 2: system identification from one broadband run, the H1 estimate of the
 * frequency response Sxy / Sxx and the coherence |Sxy|^2 / (Sxx Syy) per instance, N x nrows x 4 x (L / 2 + 1) doubles in place
 * of u [N][T][nu] and y [N][T][ny].
 *   in_row  an input row of the model, 0 <= in_row < nu.  x is that row's base-rate sample as the run sees it: the caller's u,
 *           a constant row of acme_batch_run_const, or a source of any kind (CONST included).
 *   L, hop, w   as acme_batch_set_measurement_spectrum's; the segments and their count are the spectrum's too
 *           (segments = count >= L ? (count - L) / hop + 1 : 0).
 * y is a measured output row.  Under oversampling both are the BASE-RATE signals, u before the interpolation and y after the
 * decimation: the estimate then includes the resampler's response.
 * Arithmetic, per segment and pair (instance i, measured row r) -- every operation rounded on its own, NO fused multiply-add:
 *   1. a_j = w[j] x[s hop + j], b_j = w[j] y[s hop + j], one product each.
 *   2. Z = FFT_L(a + i b), the spectrum's radix-2 decimation-in-time transform of the COMPLEX vector: its table, the
 *      bit-reversed load of both parts, its stage order and its butterfly (tr = wr br - wi bi, ti = wr bi + wi br, a + t,
 *      a - t); nothing is assumed zero.
 *   3. for k = 0 ... L / 2, with n = (L - k) mod L:
 *        Xr = 0.5 (Zr_k + Zr_n)   Xi = 0.5 (Zi_k - Zi_n)   Yr = 0.5 (Zi_k + Zi_n)   Yi = 0.5 (Zr_n - Zr_k)
 *   4. four chains per bin, each from 0.0 in segment order:
 *        xx += (Xr Xr + Xi Xi)   yy += (Yr Yr + Yi Yi)   re += (Xr Yr + Xi Yi)   im += (Xr Yi - Xi Yr)
 *      so that Sxy = re + i im = sum conj(X) Y and H1 = Sxy / Sxx.
 * As for the spectrum this fixes the VALUES, not the data flow.  PACKING: the two signals share one transform, so the rounding
 * errors of the larger enter the bins of the smaller: X and Y are each within sqrt(L) ||z||_2 (q eta / (1 - q eta) + u) (plus
 * the split's one addition) of the exact transform, with ||z||_2^2 = ||a||_2^2 + ||b||_2^2, q = log2 L and eta of DESIGN.md
 * 2.5j -- relative to ||z||, not to the signal's own norm: with |y| = 1000 |x| the X bins are off by some 10^-13 of their
 * largest, not 10^-16.  For that reason xx is kept per PAIR, not per instance: it is the xx of that pair's transform.
 * out planes in order xx, yy, re, im; no scaling by the sample rate or the window's power is applied.
 * The sums depend on nothing but the run's samples, as the spectrum's: chunk, slice and call boundaries, memory kinds, entry
 * points, y stored or NULL, the oversampling factor and ACME_OS_SLICE change none of their bits.  The measurement's own
 * accumulators and launches are what they are without it; it takes one more kernel per chunk of the window and, per pair,
 * 2 L + 4 (L / 2 + 1) doubles of device memory (a ring of the last L samples of x and one of y, and the four planes).  A fold,
 * a spectrum and a cross-spectrum may all be set together.  The cost per sample grows as the spectrum's: keep hop >= L / 8 on
 * wide batches.
 * ACME_ERR_INVALID: no measurement armed, samples already fed, L not a power of two or out of range, hop out of range, a
 * non-finite window value, in_row out of range, a model without inputs (nu == 0).  ACME_ERR_UNSUPPORTED together with a series,
 * whichever is set first.  Setting it again replaces the earlier one.  _reset_measurement zeroes the sums and the rings and keeps
 * L, hop, w, the table and in_row; arming any form or _clear_measurement removes it; acme_batch_set_matrices carries it with
 * the accumulators.  A batch without a cross-spectrum launches and allocates what it always did. */
int acme_batch_set_measurement_cross(acme_batch *b, int in_row, long long L, long long hop, const double *w /* host [L], NULL: all 1.0 */);
/* the cross-spectrum so far: out[N][nrows][4][L / 2 + 1] (may be NULL) = sums / segments, NaN everywhere while segments == 0;
 * *segments, *count: complete segments and samples measured (may be NULL).  ACME_ERR_INVALID without a cross-spectrum.  Joins a
 * pending acme_batch_run_async and synchronises the device. */
int acme_batch_get_measurement_cross(acme_batch *b, double *out, long long *segments, long long *count);
/* the same planes undivided: out[N][nrows][4][L / 2 + 1] (not NULL), the chains' sums themselves (NaN while segments == 0) */
int acme_batch_get_measurement_cross_sums(acme_batch *b, double *out);
/* the window w[L] and the table tw[L / 2][2] the kernel uses (either may be NULL) */
int acme_batch_get_measurement_cross_table(acme_batch *b, double *w, double *tw);
/* A TARGET of the window: the armed measurement (any of the three forms, any start / length, no sample fed since arming or the
 * last reset) also compares every measured row with a waveform the caller brings -- the residual y - t against a recording:
 * the error-to-signal ratio sum (y - t)^2 / sum t^2 of N candidate parameter sets against the recorded output of the real
 * device, plain and behind a first-order pre-emphasis filter; the null of a Monte-Carlo or potentiometer batch against the
 * nominal waveform; a scan of integer alignments in one batch.  7 doubles per instance and measured row in place of
 * y [N][T][ny].
 *   t        HOST array [K][nrows][P] of K target waveforms, one per measured row in the ascending order of the measurement's
 *            rows, P samples each, LOOPED; 1 <= K <= ACME_MAX_TARGETS, 1 <= P, K nrows P <= ACME_MAX_SOURCE_TABLE, every value
 *            finite.  Copied to the device by the call.
 *   which    HOST array [N] or NULL (every instance: target 0); 0 <= which[i] < K: the recording instance i is compared with
 *            (the real device recorded at K knob positions, N = K x M candidates).
 *   lag      HOST array [N] or NULL (every instance: 0); 0 <= lag[i] < P: instance i reads the target lag[i] samples ahead.
 *   preemph  the pre-emphasis coefficient c, 0 <= c < 1, finite.
 * Arithmetic, per instance i, j-th measured row and window sample m = n - start -- every product and every sum rounded on its
 * own, NO fused multiply-add anywhere, every accumulator ONE chain in sample order from 0.0:
 *   s   = (m + lag_i) mod P                      in 64-bit integers
 *   t   = tgt[(which_i nrows + j) P + s]
 *   e   = y - t
 *   See = See + e e     Stt = Stt + t t     Syt = Syt + y t     St = St + t
 *   emax = max(emax, |e|) from 0.0, NaN sticking exactly as the measurement's max does
 *   de  = e - c e_prev      dt = t - c t_prev      (e_prev = t_prev = 0.0 at m = 0)
 *   Pee = Pee + de de   Ptt = Ptt + dt dt   then e_prev = e, t_prev = t
 * The result depends on nothing but the run's samples: chunk, slice and call boundaries, host or device memory, the entry point
 * (acme_batch_run, _run_const, _run_async, _run_sources), the oversampling factor (y is the base-rate output after decimation)
 * and whether y is stored change none of its bits; e_prev and t_prev live with the accumulators and carry across chunks, slices
 * and calls.  Instance i of a per-instance arming reads, bit for bit, what a shared arming with which_i and lag_i reads.  With
 * c = 0, Pee == See and Ptt == Stt bit for bit (finite y).  The measurement's own accumulators, plan, launches and getter are
 * what they are without a target; the target takes one more kernel per chunk of the window and the table plus 9 doubles per
 * pair of device memory.  A fold, a spectrum, a cross-spectrum and a target may all be set together.
 * ACME_ERR_INVALID (the message names the argument, the instance of an entry of which or lag, the index of a non-finite target
 * value): no measurement armed, samples already fed, t null, K, P or K nrows P out of range, a non-finite target value, a
 * which[i] or lag[i] out of range, preemph out of range.  ACME_ERR_UNSUPPORTED together with a series, whichever is set first:
 * a target per window is not available.  Setting a target again replaces the earlier one.  _reset_measurement zeroes the chains
 * and the two carries and keeps the table, which, lag and c; arming any form or _clear_measurement removes the target;
 * acme_batch_set_matrices carries it with the accumulators.  A batch without a target launches, allocates and synchronises
 * what it always did. */
#define ACME_MAX_TARGETS 64
int acme_batch_set_measurement_target(acme_batch *b, const double *t /* host [K][nrows][P] */, long long K, long long P,
                                      const int *which /* host [N] or NULL */, long long *lag /* host [N] or NULL, only read */,
                                      double preemph);
/* the chains so far, undivided: out[N][nrows][7] (may be NULL) in the order See, Stt, Syt, St, emax, Pee, Ptt (the tests pin
 * them with ==; sums of separate runs can be added); *count: samples measured, as acme_batch_get_measurement counts them (may
 * be NULL).  A window nothing has reached reads 0.0 with count 0.  ACME_ERR_INVALID without a target.  Joins a pending
 * acme_batch_run_async and synchronises the device. */
int acme_batch_get_measurement_target(acme_batch *b, double *out, long long *count);
/* A WEIGHTING ahead of the measurement: the armed measurement (any form -- single window, per instance, bins, a series, with
 * or without a fold, a spectrum, a cross-spectrum, a target --, no sample fed since arming or the last reset) reads every
 * measured row through one cascade of S second-order sections, shared by all instances and rows: a band limit ahead of a
 * THD+N reading, A, C or ITU-R 468 weighting ahead of a noise level, the K filter of BS.1770 ahead of the mean squares of a
 * series of 400 ms blocks, a DC blocker ahead of any RMS, a pre-emphasis of the caller's ahead of the target's error-to-signal
 * ratio -- none of which needs y [N][T][ny] stored.
 *   sos      HOST array [S][5], per section b0 b1 b2 a1 a2 of H(z) = (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2) (a0 = 1);
 *            every value finite.  Copied by the call.
 *   S        1 ... ACME_MAX_WEIGHTING_SECTIONS
 * The filter runs on EVERY base-rate output sample since arming, from sample 0 and not only inside the window (a transient has
 * decayed by `start`), after the decimation of an oversampled batch.  Arithmetic, transposed direct form II, per instance,
 * measured row, sample x = y and section k = 0 ... S - 1 in order -- every product and every sum rounded on its own, NO fused
 * multiply-add, the parentheses as written:
 *   v  = b0 x + s1
 *   s1 = (b1 x - a1 v) + s2
 *   s2 = b2 x - a2 v
 *   x  = v                                       for the next section
 * with s1 = s2 = 0.0 at arming and at a reset; the last section's v is the weighted sample w.  Subnormals are kept (the kernel
 * leaves the fp64 denormal mode alone); a NaN sticks in the states of its own (instance, row) pair and touches no other.
 * Every form reads w where it read y: the moments, min and max, the harmonics and bins, the windows of a series, the slots of
 * a fold, the segments of a spectrum and of a cross-spectrum, the target's e = w - t.  The INPUT row of a cross-spectrum stays
 * unweighted: H then includes the weighting's response, the coherence is what it is without a weighting.  The target's t is
 * compared as brought (weight a recording on the host with the same arithmetic first).  A stored y is the raw output.
 * The result depends on nothing but the run's samples: chunk, slice and call boundaries, host or device memory, the entry
 * point, the oversampling factor and whether y is stored change none of its bits; the states live with the accumulators and
 * carry across chunks, slices and calls.  The weighting takes one more kernel per slice, one slice of weighted rows
 * [N][n][nrows] and 2 S doubles per pair of device memory; the measurement kernels are what they are without it.
 * ACME_ERR_INVALID (the message names the argument, and the entry of a non-finite coefficient): no measurement armed, samples
 * already fed, sos null, S out of range, a non-finite coefficient.  Setting a weighting again replaces the earlier one.
 * _reset_measurement zeroes the states and keeps the coefficients; arming any form or _clear_measurement removes the
 * weighting; acme_batch_set_matrices carries it with the accumulators.  A batch without a weighting launches, allocates and
 * synchronises what it always did. */
#define ACME_MAX_WEIGHTING_SECTIONS 8
int acme_batch_set_measurement_weighting(acme_batch *b, const double *sos /* host [S][5]: b0 b1 b2 a1 a2 */, int S);
/* the cascade as set: sos[8][5] (may be NULL; the rows from S on are 0.0) and *S (may be NULL).  ACME_ERR_INVALID without a
 * weighting. */
int acme_batch_get_measurement_weighting(acme_batch *b, double *sos /* [8][5] or NULL */, int *S);
/* An ENSEMBLE of the window: the armed measurement (any of the three forms with a BOUNDED window, length > 0, no sample fed
 * since arming or the last reset) also reduces over the INSTANCES at one time sample, where every other form reduces over
 * time for one instance -- the band of the output waveform over the draws of a Monte-Carlo batch (mean, +- sigma, min / max
 * envelope), which draw is the worst case at each point of the period, the same per cell of a grid with M draws a cell, the
 * ensemble average of a batch in which every instance hears its own noise row; with groups of one member, the waveform of a
 * few chosen instances of a y = NULL run.  6 values per group, measured row and recorded sample in place of y [N][T][ny].
 *   group    HOST array [N] or NULL (every instance in group 0); group[i] in 0 ... G - 1: the group of instance i, -1: in no
 *            group.  Groups are arbitrary (interleaved, not contiguous, of unequal size); a group may be empty.
 *   G        the number of groups, >= 1
 *   stride   >= 1: window sample m = n - start is recorded iff m mod stride == 0, in slot e = m / stride;
 *            E = ceil(length / stride) slots; G nrows E <= ACME_MAX_ENSEMBLE.
 * Arithmetic, per group g, j-th measured row and slot e: six values, each ONE chain over the group's members in ASCENDING
 * INSTANCE ORDER i, every product and every sum rounded on its own, NO fused multiply-add; v is the value the other forms see
 * (the weighted row behind a weighting, the base-rate row after the decimation of an oversampled batch):
 *   S = S + v                                    from 0.0
 *   q = v v;  Q = Q + q                          from 0.0
 *   if (v < mn || v != v) { mn = v; imin = i; }  from +inf and -1
 *   if (v > mx || v != v) { mx = v; imax = i; }  from -inf and -1
 * -- the measurement's min and max with the index carried: the FIRST member that attains an extreme keeps it; a NaN sticks in
 * all four values of its (group, row, slot), and imin == imax name the NaN member (with several NaN members at one sample, the
 * last of them, as the rule reads).  A group of ONE member therefore returns S = 0.0 + y: the stored y bit for bit, except
 * that -0.0 reads +0.0 (min and max keep the sign).  A slot is written exactly once, by the chunk that holds its sample;
 * nothing carries across chunks, slices or calls.  Slots not reached yet and empty groups read the start values.  The
 * result depends on nothing but the run's samples: chunk, slice and call boundaries, host or device memory, the entry point,
 * the oversampling factor and whether y is stored change none of its bits.  The measurement's own accumulators, plan,
 * launches and getter are what they are without an ensemble; it takes one more kernel per chunk of the window, the member
 * list and 6 x 8 bytes per (group, row, slot) of device memory.  A fold, a spectrum, a cross-spectrum, a target, a weighting
 * and an ensemble may all be set together.
 * ACME_ERR_INVALID (the message names the argument, and the instance of an entry of group): no measurement armed, samples
 * already fed, an unbounded window (length == 0), G < 1, stride < 1, G nrows E beyond the cap, a group[i] outside -1 ... G - 1.
 * ACME_ERR_UNSUPPORTED together with a series, whichever is set first.  Setting an ensemble again replaces the earlier one.
 * _reset_measurement returns every slot to the start values and keeps group, G and stride; arming any form or
 * _clear_measurement removes the ensemble; acme_batch_set_matrices carries it with the accumulators.  A batch without an
 * ensemble launches, allocates and synchronises what it always did. */
#define ACME_MAX_ENSEMBLE 16777216
int acme_batch_set_measurement_ensemble(acme_batch *b, const int *group /* host [N]: 0 ... G - 1, -1: in no group; NULL: all in group 0 */,
                                        int G, long long stride);
/* the chains so far, undivided (each may be NULL): out[G][nrows][E][4] in the order S, Q, min, max; arg[G][nrows][E][2] the
 * instances imin, imax (-1: no member); members[G] the groups' sizes; *filled the number of slots recorded so far,
 * ceil(samples measured / stride).  ACME_ERR_INVALID without an ensemble.  Joins a pending acme_batch_run_async and
 * synchronises the device. */
int acme_batch_get_measurement_ensemble(acme_batch *b, double *out /* [G][nrows][E][4] */, long long *arg /* [G][nrows][E][2] */,
                                        long long *members /* [G] */, long long *filled);
/* A HISTOGRAM of the window: the armed measurement (any of the three forms, any start / length, bounded or not, no sample fed
 * since arming or the last reset) also counts HOW THE AMPLITUDE IS DISTRIBUTED, per instance and measured row -- the share of
 * the window an output spends above a level (time in clipping across a drive sweep, the probability of overload across
 * Monte-Carlo draws), the median and any percentile (L10 / L50 / L90 of a noise-loaded run, the 99.9 % level as a robust peak),
 * the density itself (a clipper's pile-up at the rails, a comparator's two modes, asymmetry, dead zones), and the rectified
 * form of each.  B + 3 integer counters per pair in place of y [N][T][ny].
 *   bins     B, 1 ... ACME_MAX_HIST_BINS; N nrows (B + 3) <= ACME_MAX_HISTOGRAM
 *   mode     ACME_HIST_SIGNED: x = v;  ACME_HIST_ABS: x = |v|.  v is the value the other forms see (the weighted row behind a
 *            weighting, the base-rate row after the decimation of an oversampled batch)
 *   lo, hi   the range of every instance, finite, lo < hi -- used iff lo_i and hi_i are NULL
 *   lo_i, hi_i   HOST arrays [N], both or neither: instance i's own range (a drive sweep's range scales with the level);
 *            copied by the call, lo and hi are then ignored
 * The scale of instance i is formed ONCE, on the host, with two roundings -- d = hi_i - lo_i;  s_i = (double)B / d -- and
 * stored; the getter hands it back, so that a replay uses the same bits.  Per sample EXACTLY ONE of the B + 3 counters of its
 * (instance, row) goes up by one:
 *   if (x != x)          NAN   += 1
 *   else if (x < lo_i)   UNDER += 1
 *   else if (x >= hi_i)  OVER  += 1
 *   else { t = x - lo_i;  q = t * s_i;       each rounded on its own, NO fused multiply-add
 *          k = (long long)q;                 truncation; q >= 0 here
 *          if (k > B - 1) k = B - 1;         q can round up to B just below hi_i
 *          BIN[k] += 1 }
 * Bins are half-open: x == lo_i is bin 0, x == hi_i is OVER; -0.0 with lo_i = 0 is bin 0; +inf is OVER and -inf UNDER (in
 * the ABS mode both are OVER); a NaN -- every sample of an instance from its first_nonfinite sample on -- counts in NAN and
 * touches no other pair.  Bin k nominally covers [lo_i + k / s_i, lo_i + (k + 1) / s_i); AT an edge the two roundings of t and
 * q decide on which side a value falls, and the rule above is the definition.  Counters are 64-bit integers, so the result
 * depends on nothing but the run's samples: chunk, slice and call boundaries, host or device memory, the entry point
 * (acme_batch_run, _run_const, _run_async, _run_sources), the oversampling factor, a weighting beyond what it feeds as v and
 * whether y is stored change none of its bits.  The measurement's own accumulators, plan, launches and getter are what they
 * are without a histogram; it takes one more kernel per chunk of the window and 8 (B + 3) bytes per pair plus 24 bytes per
 * instance of device memory.  A fold, a spectrum, a cross-spectrum, a target, a weighting, an ensemble and a histogram may
 * all be set together.
 * ACME_ERR_INVALID (the message names the argument, and the instance of an entry of lo_i / hi_i): no measurement armed,
 * samples already fed, bins outside 1 ... ACME_MAX_HIST_BINS, an unknown mode, a non-finite bound, lo_i >= hi_i, hi_i - lo_i
 * overflowing to infinity (or so small that B / d does), one array without the other, N nrows (B + 3) beyond
 * ACME_MAX_HISTOGRAM.  ACME_ERR_UNSUPPORTED together with a series, whichever is set first: a histogram per window is not
 * available.  Setting a histogram again replaces the earlier one.  _reset_measurement zeroes the counters and keeps bins,
 * mode and the ranges; arming any form or _clear_measurement removes the histogram; acme_batch_set_matrices carries it with
 * the accumulators; the refusal together with acme_batch_set_isolation is the measurement's own.  A batch without a histogram
 * launches, allocates and synchronises what it always did.
 * Out of scope: ranges per ROW (one range per instance serves all its measured rows); logarithmic (dB) bins -- log is not
 * reproducible bit for bit; automatic ranging -- the recipe is a first run with the plain measurement for min / max, then
 * _reset_measurement and the histogram. */
#define ACME_HIST_SIGNED 0
#define ACME_HIST_ABS    1
#define ACME_MAX_HIST_BINS 4096
#define ACME_MAX_HISTOGRAM 268435456        /* N nrows (B + 3) counters at most */
int acme_batch_set_measurement_histogram(acme_batch *b, int bins, int mode, double lo, double hi,
                                         const double *lo_i /* host [N] or NULL */, const double *hi_i /* host [N] or NULL */);
/* the counters so far (each argument may be NULL): counts[N][nrows][B + 3] -- [0] UNDER, [1 ... B] BIN[0 ... B - 1], [B + 1]
 * OVER, [B + 2] NAN --, range[N][3] = lo_i, hi_i, s_i as stored, *count the samples measured, as acme_batch_get_measurement
 * counts them: the B + 3 counters of every pair sum to it exactly.  ACME_ERR_INVALID without a histogram.  Joins a pending
 * acme_batch_run_async and synchronises the device. */
int acme_batch_get_measurement_histogram(acme_batch *b, long long *counts /* [N][nrows][B + 3] */,
                                         double *range /* [N][3]: lo_i, hi_i, s_i */, long long *count);
/* EVENTS of the window: the armed measurement (any of the three forms, any start / length, bounded or not, no sample fed
 * since arming or the last reset) also records WHEN the measured rows cross levels, per instance, measured row and level -- the
 * `.measure TRIG / TARG / WHEN` questions of a circuit simulator: the rise and fall time of a step response between its 10 %
 * and 90 % levels, the delay to a threshold, the settling time (the last time the output leaves a band), the frequency of an
 * oscillating output from its zero crossings to a fraction of a sample, the duty cycle of a clipped or comparator output, how
 * often a noisy output chatters across a trip level with a Schmitt hysteresis or without.  A few integers and sample pairs per
 * (instance, row, level) in place of y [N][T][ny].
 *   C        levels per instance, 1 ... ACME_MAX_EVENT_LEVELS
 *   lo, hi   HOST arrays [C][N], copied by the call: level c of instance i at [c * N + i]; every value finite, lo <= hi.
 *            lo == hi is a plain comparator, lo < hi a Schmitt trigger
 *   E        the first events recorded per direction, 0 ... ACME_MAX_EVENT_SLOTS; N nrows C (E + 1) <= ACME_MAX_EVENTS
 * Every triple (instance i, measured row r, level c) has a STATE, UNKNOWN, LOW or HIGH, UNKNOWN at the window's first sample.
 * Window sample m counts from 0 at `start`; its value v is the value the other forms see (the weighted row behind a weighting,
 * the base-rate row after the decimation of an oversampled batch).  Per sample:
 *   if      (v >= hi) next = HIGH
 *   else if (v <= lo) next = LOW
 *   else              next = state            inside the band, or NaN: keep
 *   RISE at m  iff state == LOW  and next == HIGH
 *   FALL at m  iff state == HIGH and next == LOW
 * Leaving UNKNOWN is no event: an event never falls on m = 0, and v[m - 1] exists for every event.  The device performs NO
 * floating-point arithmetic, only comparisons.  Per triple it keeps
 *   five 64-bit counters, in this order: RISE and FALL, the events; HIGH and LOW, the samples whose state AFTER the sample is
 *            HIGH or LOW (a NaN sample counts in the state it keeps); UNKNOWN, the samples after which the state is still
 *            unknown.  HIGH + LOW + UNKNOWN == count for every triple;
 *   E + 1 event records per direction (0: rises, 1: falls): slots 0 ... E - 1 the first E events in time order, slot E the LAST
 *            event so far (it equals slot n - 1 while the direction has had n <= E events).  A record is (m, a, b) = (the
 *            window sample as a 64-bit integer, v[m - 1], v[m]), the values copied bit for bit; an empty slot is (-1, 0.0, 0.0).
 *            The HOST forms the time to a fraction of a sample, t = (m - 1) + (thr - a) / (b - a) with thr = hi for a rise and
 *            lo for a fall, t = m where a is NaN: no quotient has to be bit-exact anywhere;
 *   the state and the last window sample's value, carried across chunks, slices and calls.
 * Integers and copied values, so the result depends on nothing but the run's samples: T1 then T2 samples equal one run of
 * T1 + T2, and chunk, slice and call boundaries, host or device memory, the entry point (acme_batch_run, _run_const,
 * _run_async, _run_sources), the oversampling factor, a weighting beyond what it feeds as v and whether y is stored change
 * none of its bits.  The measurement's own accumulators, plan, launches and getter are what they are without events, and so are
 * those of a fold, a spectrum, a cross-spectrum, a target, a weighting, an ensemble and a histogram set beside them; events
 * take one more kernel per chunk of the window.
 * ACME_ERR_INVALID (the message names the argument, and the level and instance of an entry of lo / hi): no measurement armed,
 * samples already fed, C outside 1 ... ACME_MAX_EVENT_LEVELS, E outside 0 ... ACME_MAX_EVENT_SLOTS, lo or hi NULL, a
 * non-finite level, lo > hi, N nrows C (E + 1) beyond ACME_MAX_EVENTS (the product equal to it is accepted).
 * ACME_ERR_UNSUPPORTED together with a series, whichever is set first.  Setting events again replaces the earlier ones.
 * _reset_measurement zeroes the counters, empties the slots and returns the states to UNKNOWN; it keeps C, E and the levels.
 * Arming any form or _clear_measurement removes the events; acme_batch_set_matrices carries them with the accumulators.  A batch
 * without events launches, allocates and synchronises what it always did.
 * Out of scope: levels per ROW (an instance's levels serve all its measured rows); events per window of a series; more than
 * the first E and the last event of a direction -- count them, or use a longer E on a shorter window. */
#define ACME_MAX_EVENT_LEVELS 8
#define ACME_MAX_EVENT_SLOTS 16
#define ACME_MAX_EVENTS 16777216            /* N nrows C (E + 1) records per direction at most */
#define ACME_EVENT_RISE 0                   /* the counters of a triple, in the getter's order */
#define ACME_EVENT_FALL 1
#define ACME_EVENT_HIGH 2
#define ACME_EVENT_LOW 3
#define ACME_EVENT_UNKNOWN 4
int acme_batch_set_measurement_events(acme_batch *b, int C, const double *lo /* host [C][N] */, const double *hi /* host [C][N] */,
                                      int E);
/* the events so far (each argument may be NULL): counts[N][nrows][C][5] -- RISE, FALL, HIGH, LOW, UNKNOWN --,
 * idx[N][nrows][C][2][E + 1] the records' window samples m (rises, then falls; -1: empty), ab[N][nrows][C][2][E + 1][2] their
 * v[m - 1] and v[m], *count the samples measured, as acme_batch_get_measurement counts them.  ACME_ERR_INVALID without events.
 * Joins a pending acme_batch_run_async and synchronises the device. */
int acme_batch_get_measurement_events(acme_batch *b, long long *counts /* [N][nrows][C][5] */,
                                      long long *idx /* [N][nrows][C][2][E + 1] */, double *ab /* [N][nrows][C][2][E + 1][2] */,
                                      long long *count);
/* switch the measurement off (y = NULL is refused again) */
int acme_batch_clear_measurement(acme_batch *b);
/* zero the accumulators and restart the window's clock (the armed parameters stay) */
int acme_batch_reset_measurement(acme_batch *b);
/* out: [N][nrows][4 + 2H] doubles as above (may be NULL); *count: samples measured (may be NULL).  Joins a pending
 * acme_batch_run_async and synchronises the device. */
int acme_batch_get_measurement(acme_batch *b, double *out, long long *count);

/* Sources: input signals generated on the device.  In a level sweep, a potentiometer grid, a Monte-Carlo run the input of
 * instance i is a known function of a few numbers and one shared waveform; a row with a SOURCE needs no u from the caller --
 * the library generates it time slice by time slice (one slice of scratch; with a measurement armed and y = NULL a sweep owns
 * no [N][T] array anywhere, and nothing but parameters and results crosses the bus).
 *   source clock  while at least one row has a source the batch has a clock n (64-bit, base-rate samples): 0 when the first
 *                 source is armed, advanced by T by every source run, carried from call to call
 *   kinds         value of the row at clock n, instance i
 *     ACME_SOURCE_CONST   offset_i
 *     ACME_SOURCE_SINE    fma(amp_i, sin(th), offset_i),  th = 2 pi kappa / f_den,
 *                         kappa = (f_num_i n + phase_i) mod f_den taken to (-f_den / 2, f_den / 2]: the phase reduced exactly in
 *                         64-bit integers (n mod f_den first), the angle with two roundings (the quotient kappa / f_den, its
 *                         product with 2 pi) as the measurement's twiddles; 0 <= f_num_i, phase_i < f_den < 2^31.  The
 *                         frequency is f_num_i / f_den x the base sample rate per instance: a frequency sweep is one batch
 *     ACME_SOURCE_TABLE   fma(amp_i, w[n mod P], offset_i): a looped wavetable w[P], 1 <= P <= ACME_MAX_SOURCE_TABLE (a chirp,
 *                         a multitone, a recorded bar: P = its length)
 *     ACME_SOURCE_MULTISINE  a sum of `tones` (1 ... ACME_MAX_SOURCE_TONES) sines, ONE chain in tone order: v = offset_i, then
 *                         v = fma(amp_ki, sin(th_k), v) for k = 0 ... tones - 1, th_k = 2 pi kappa_k / f_den with
 *                         kappa_k = (f_num_ki n + phase_ki) mod f_den reduced and rounded exactly as SINE's.  One tone is the
 *                         SINE row bit for bit.  Per-instance tone frequencies, levels and relative phases: a two-tone
 *                         intermodulation sweep (the pair's centre, spacing, ratio) is one batch.  The per-tone arrays are
 *                         [tones][N]: tone k of instance i at [k * N + i]
 *     ACME_SOURCE_NOISE   independent, reproducible random rows, COUNTER BASED: the value at clock n depends on (stream_i, row,
 *                         q = n div hold) alone -- never on what was generated before, on the call boundaries or on the memory
 *                         kind; a render at clock 2^62 costs what one at 0 costs.  One Philox4x32-10 block (multipliers
 *                         D2511F53, CD9E8D57; key increments 9E3779B9, BB67AE85) per (instance, row, q): counter (q mod 2^32,
 *                         q div 2^32, row, 0), key (stream_i mod 2^32, stream_i div 2^32) with stream_i read as unsigned 64 bit,
 *                         outputs r0 ... r3; the 53-bit draw x = r0 + 2^32 (r1 mod 2^21), then
 *                           ACME_NOISE_UNIFORM   fma(amp_i, U, offset_i), U = (2 x + 1 - 2^53) 2^-53: exact, symmetric about 0,
 *                                                never 0, in (-1, 1); variance 1/3
 *                           ACME_NOISE_GAUSSIAN  fma(amp_i, g, offset_i), g = sqrt(-2 log(u1)) sin(th), u1 = (x + 1) 2^-53 in
 *                                                (0, 1], th = 2 pi kappa / 2^32 with kappa = r2 taken to (-2^31, 2^31] (the SINE
 *                                                row's angle); variance 1
 *                         hold (1 ... 2^31 - 1): the row is a sample-and-hold of the draw over blocks of `hold` samples aligned
 *                         to the CLOCK (1: white noise at the base rate; larger: stepped random values, a jumping pot).
 *                         stream: a HOST array of N entries or NULL (stream_i = i); equal streams on one row render equal
 *                         sequences, the same stream on two rows independent ones
 *     ACME_SOURCE_PULSE   fma(amp_i, e, offset_i), e a per-instance TRAPEZOID envelope: five integers per instance -- period P_i
 *                         (1 ... 2^31 - 1), delay_i (0 ... P_i - 1), rise_i, on_i, fall_i >= 0 with rise + on + fall <= P_i --
 *                         and j = (n - delay_i) mod P_i, reduced exactly in 64-bit integers (n mod P_i first: valid for clocks
 *                         up to 2^62):
 *                           e = (double)j / (double)rise                         j < rise
 *                               1.0                                              rise <= j < rise + on
 *                               (double)(rise + on + fall - j) / (double)fall    rise + on <= j < rise + on + fall
 *                               0.0                                              otherwise
 *                         The conversions are exact, a ramp sample is ONE correctly rounded division: with the fma two roundings
 *                         at most, the row is reproducible bit for bit.  rise = fall = 0: high for exactly `on` samples per
 *                         period, the duty cycle on / P exactly.  rise > 0: the sampled continuous trapezoid, 0 at j = 0, 1 at
 *                         j = rise when on > 0 (or on = 0 and fall > 0; with on = fall = 0 it never reaches 1).  A step is a
 *                         pulse of P = 2^31 - 1; a ramp-and-hold of a pot row a long rise on that step; a PWM or duty sweep, an
 *                         edge-time sweep, a delay scan are each one batch
 *     ACME_SOURCE_BURST   a tone burst: g = amp_i e (one rounded product), then fma(g, sin(th), offset_i) with e PULSE's
 *                         envelope and th exactly SINE's angle from (f_num_i n + phase_i) mod f_den.  Where e = 1 the row is the
 *                         SINE row bit for bit, where e = 0 it is offset_i.  The tone runs with the CLOCK, it does not restart per
 *                         burst: a burst starts at a zero crossing when delay and P are multiples of the tone's period
 *                         shape: a HOST array [5][N] -- period, delay, rise, on, fall; entry k of instance i at shape[k * N + i]
 *   parameters   amp, offset, f_num, phase: HOST arrays of N entries, copied to the device by the call (parameters, not
 *                 signals); NULL = the same default for every instance (amp 1, the others 0).  w: a host array of P entries.
 *                 (f_num and phase are only read.)
 * DEFINING PROPERTY: acme_batch_run_sources produces, bit for bit, what acme_batch_run produces on the materialised u --
 * what acme_batch_render_sources writes --: outputs, state, extrapolation origins, acme_report, measurement accumulators,
 * oversampling histories; in host and device memory, with y stored or y = NULL (measurement armed), in split calls (T1 then
 * T2 = one run of T1 + T2), asynchronously, with the balancing on or off.  On an oversampled batch a sourced row is generated
 * at the BASE rate and then treated as a caller's row is: interpolated, or held if its bit is in held_rows; a CONST row is
 * always held (as the constant rows of acme_batch_run_const are).  An ideal edge of a PULSE or BURST row (rise = 0 or
 * fall = 0) wants the row HELD: interpolated, the band-limiting filter rings on it.
 * Runs go slice by slice on the launch stream (the source kernel, csrc/acme_source.h, ahead of the slice's interpolation /
 * run kernel); host buffers take the staged slice pipeline, never the streamed path of acme_batch_set_host_retention.  While
 * a row has a source, acme_batch_run, _run_const and _run_async return ACME_ERR_INVALID (rows of a full u would be silently
 * ignored).  acme_batch_set_matrices, _set_state, _reset_report, _set_oversampling and the measurement calls leave the sources
 * and the clock alone.  Not together with acme_batch_set_isolation (ACME_ERR_UNSUPPORTED either way round), nor on models of
 * more than 64 input rows.  No source armed: no launch, allocation or synchronisation of any run changes. */
#define ACME_SOURCE_CONST 1
#define ACME_SOURCE_SINE 2
#define ACME_SOURCE_TABLE 3
#define ACME_SOURCE_MULTISINE 4
#define ACME_SOURCE_NOISE 5
#define ACME_SOURCE_PULSE 6
#define ACME_SOURCE_BURST 7
#define ACME_NOISE_UNIFORM 0
#define ACME_NOISE_GAUSSIAN 1
#define ACME_MAX_SOURCE_TABLE 16777216
#define ACME_MAX_SOURCE_TONES 4
/* give input row `row` a source (replacing the one it has).  Validates its arguments (ACME_ERR_INVALID: row beyond the model's
 * inputs, f_den or P out of range, an f_num_i or phase_i outside 0 ... f_den - 1, non-finite amp / offset).  Completes the
 * batch's outstanding work first. */
int acme_batch_set_source_const(acme_batch *b, int row, const double *offset);
int acme_batch_set_source_sine(acme_batch *b, int row, long long f_den, long long *f_num, long long *phase,
                               const double *amp, const double *offset);
int acme_batch_set_source_table(acme_batch *b, int row, const double *w, long long P, const double *amp,
                                const double *offset);
/* f_num (required), phase, amp: [tones][N]; offset: [N].  ACME_ERR_INVALID also for tones outside 1 ... ACME_MAX_SOURCE_TONES
 * and a null f_num; an f_num or phase out of range is named by tone and instance. */
int acme_batch_set_source_multisine(acme_batch *b, int row, long long f_den, int tones, long long *f_num, long long *phase,
                                    const double *amp, const double *offset);
/* stream: [N] or NULL (stream_i = i), only read; amp, offset: [N] or NULL.  ACME_ERR_INVALID also for a dist that is neither
 * ACME_NOISE_UNIFORM nor ACME_NOISE_GAUSSIAN and a hold outside 1 ... 2^31 - 1. */
int acme_batch_set_source_noise(acme_batch *b, int row, int dist, long long hold, long long *stream, const double *amp,
                                const double *offset);
/* shape: [5][N] (period, delay, rise, on, fall), required, only read; amp, offset: [N] or NULL.  ACME_ERR_INVALID, naming the
 * instance, also for a null shape, a period outside 1 ... 2^31 - 1, a delay outside 0 ... period - 1, a negative rise, on or
 * fall and rise + on + fall > period; the burst adds the sine's checks of f_den, f_num and phase (the tone's).  A refused call
 * leaves the row as it was. */
int acme_batch_set_source_pulse(acme_batch *b, int row, long long *shape, const double *amp, const double *offset);
int acme_batch_set_source_burst(acme_batch *b, int row, long long *shape, long long f_den, long long *f_num,
                                long long *phase, const double *amp, const double *offset);
/* the row is the caller's again; row < 0: every row. With the last source the clock goes (the next first source starts
 * it at 0). */
int acme_batch_clear_source(acme_batch *b, int row);
/* the source clock (n >= 0); ACME_ERR_INVALID while no row has a source */
int acme_batch_set_source_clock(acme_batch *b, long long n);
int acme_batch_get_source_clock(acme_batch *b, long long *n);
/* run! with the sourced rows generated: u_var [N][T][nu_var] holds only the rows WITHOUT a source, in row order (the layout
 * of acme_batch_run_const); NULL when every row has a source.  y, T, mem, stream as acme_batch_run (y = NULL only while a
 * measurement is armed).  ACME_ERR_INVALID when no row has a source.  The _async form: as acme_batch_run_async, joined by
 * acme_batch_wait. */
int acme_batch_run_sources(acme_batch *b, const double *u_var, double *y, long long T, int mem, void *stream);
int acme_batch_run_sources_async(acme_batch *b, const double *u_var, double *y, long long T, int mem, void *stream);
/* write the [N][T][nu] input a source run of T samples would feed from the current clock -- sourced rows generated, the
 * others taken from u_var, zero where u_var is NULL --; advances neither the clock nor the model.  mem / stream: where
 * u_var and u_out live, as acme_batch_run. */
int acme_batch_render_sources(acme_batch *b, const double *u_var, double *u_out, long long T, int mem, void *stream);

/* acme_batch_run without blocking the caller: the same run on a worker thread of the library (a
 * host-buffer run drives its time-slice pipeline from there).  ONE host thread can thereby keep one
 * batch per GPU of a node busy -- start all, then acme_batch_wait each -- which is how a single
 * (Julia) process uses the 8 GPUs of a node without any collective: contiguous instance ranges, every
 * batch reading and writing its own slice of the caller's u / y.  At most one run is in flight per
 * batch; every other entry point taking the batch first waits for it.  u / y must stay valid until
 * acme_batch_wait, which returns the run's status (acme_last_error() then holds its message). */
int acme_batch_run_async(acme_batch *b, const double *u, double *y, long long T, int mem,
                         void *stream);
int acme_batch_wait(acme_batch *b);

/* Isolation of slow instances.  A launch lasts as long as its slowest wave, and every wave is one serial recurrence
 * over the samples: ONE pathological cell of a sweep -- say a potentiometer at an end stop that makes the model
 * singular, where the solver stack fails after ~900 Newton iterations per sample while every other cell needs 3 --
 * holds the results of all instances back by its own, hundreds of times longer, run.  With a threshold > 0 the
 * instances that needed more than `iters_per_sample` Newton iterations per sample over the batch's previous run are
 * launched on their own, on a stream of the library's; the others run on the caller's stream as if the slow ones were
 * not there.  What an instance computes does not depend on the group it runs in (bit-identical results).  A
 * device-pointer run (ACME_MEM_DEVICE) then completes on the caller's stream for the FAST instances only;
 * acme_batch_wait (or any entry point that reads the batch) completes the slow ones.  Host-buffer runs return
 * complete, as ever.  The first run of a batch is never split (nothing is known yet); groups are re-formed between
 * runs while no launch of the slow group is in flight.  0 switches the isolation off (default).  Not for batches the
 * lane-per-instance or generic kernels run. */
int acme_batch_set_isolation(acme_batch *b, double iters_per_sample);

/* Placement of the waves by their measured cost.  Two blocks of a launch share a compute unit and a launch ends with
 * its slowest SIMD; before a launch (at most once per 4 096 samples) two small kernels on the launch's own stream rank
 * the waves -- groups of 4 consecutive instances -- by the Newton iterations they needed since the last placement and
 * deal them to the launch's slots so that heavy and light waves share a SIMD (headline grid: 1.6 % over seconds 1-4 of a
 * signal, when the cells' costs differ most; nothing in the long steady state; tools/balance_probe.py).  No host synchronisation; what an instance computes does not depend on where it runs
 * (bit-identical results).  mode: -1 = the library decides (default: on when the launch has more waves than one round
 * of blocks holds), 0 = off, 1 = on.  Not for batches the lane-per-instance or generic kernels run, nor
 * while acme_batch_set_isolation is in force. */
int acme_batch_set_balance(acme_batch *b, int mode);
/* diagnostics: the placement the last launch used -- *n_slots instance slots (a multiple of 4: a wave has four), slot ->
 * instance in slot_to_instance[*n_slots], -1 for a slot left empty (an incomplete last wave's); at most 4 N slots; the
 * identity over N slots while nothing has been placed.
 * Either pointer may be null.  Completes the batch's outstanding work first. */
int acme_batch_get_placement(acme_batch *b, int *slot_to_instance, long long *n_slots);

/* The solver plugin contract, batched (src/solvers.jl:207-236, 268-302): for every instance
 *   z = solve(solver, p); converged = hasconverged(solver); iters = needediterations(solver)
 * on sub-problem `sub` (0-based): p is [N][np_sub], z is [N][nn_sub], converged/iters are [N].  Like the reference's
 * solver objects the call uses and updates the instance's extrapolation origin; x is not
 * touched and nothing is added to the run reports.  mem/stream as for acme_batch_run. */
int acme_batch_solve(acme_batch *b, int sub, const double *p, double *z, int *converged,
                     int *iters, int mem, void *stream);

/* get_extrapolation_jacobian(solver) (src/solvers.jl:198-201; what linearize builds the small-signal
 * model from, :407-414) for every instance: jac is [N][np_sub][nn_sub], i.e. per instance the
 * nn x np matrix  -(J \ Jp)  = dz/dp at the instance's extrapolation origin (last_p, last_z) of
 * sub-problem `sub`, column-major like Julia's Matrix{Float64}; NaN where J is singular there.  The
 * origin is re-linearised on the device (set_extrapolation_origin, :183-196, with the columns of Jp
 * riding along in the elimination); the batch's state is not modified.  mem/stream as for
 * acme_batch_run. */
int acme_batch_get_extrapolation_jacobian(acme_batch *b, int sub, double *jac, int mem, void *stream);

/* milliseconds the last acme_batch_run kernel took on the device (HIP events recorded on
 * the launch stream); synchronises with that launch */
int acme_batch_last_kernel_ms(acme_batch *b, float *ms);
/* accumulated device time and count of all launches since the last reset (HIP events on
 * the launch stream around every kernel); synchronises with the pending launches */
int acme_batch_kernel_time(acme_batch *b, double *ms_total, long long *launches, int reset);

/* per-instance reports, reports[n_instances]; synchronises */
int acme_batch_get_report(acme_batch *b, acme_report *reports);
int acme_batch_reset_report(acme_batch *b);

/* set_resabstol! (src/solvers.jl:181,262) */
int acme_batch_set_resabstol(acme_batch *b, double tol);

/* model.x and get/set_extrapolation_origin (src/solvers.jl:183-198) for all instances:
 * x is [N][nx], p is [N][sum np_k], z is [N][sum nn_k] (sub-problems concatenated in order);
 * NULL pointers are skipped */
int acme_batch_get_state(acme_batch *b, double *x, double *p, double *z);
int acme_batch_set_state(acme_batch *b, const double *x, const double *p, const double *z);

#ifdef __cplusplus
}
#endif
#endif
