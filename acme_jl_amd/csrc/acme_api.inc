// acme_api.inc -- C ABI implementation (include/acme_hip.h), written against a tiny device
// backend `be::` so that the HIP library (acme_hip.hip) and the CPU wave emulator used by the
// GPU-less unit tests (tests/emu) share every line of host logic.  Included, not compiled alone.
#include "acme_resample.h"
#include "acme_measure.h"
#include "acme_source.h"
// ------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                             \
    do {                                                                                         \
        int e_ = (int)(expr);                                                                  \
        if (e_ != 0) return fail(ACME_ERR_HIP, std::string(#expr) + ": " + be::err_string(e_)); \
    } while (0)

struct acme_model {
    HostModel h;
};

// Every entry point that touches the device runs on the batch's device and leaves the caller's
// current device as it found it.
struct DeviceGuard {
    int prev = -1, rc = 0;
    explicit DeviceGuard(int dev) {
        if (be::get_device(&prev) != 0) prev = -1;
        if (prev != dev) rc = be::set_device(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)be::set_device(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define ON_DEVICE(b)                     \
    DeviceGuard guard_((b)->device);     \
    HIPCHK(guard_.rc)

struct acme_batch {
    Packed P;
    const KernelEntry *k = nullptr;
    const KernelFns *kf = nullptr;   // the kernels the batch runs: k->lds, or k->low when its images do not fit LDS
    bool low = false;
    long long N = 0;
    acme_options o{};
    int device = 0;
    double *d_image = nullptr, *d_rowc = nullptr, *d_state = nullptr, *d_lanec = nullptr;
    int *d_rowi = nullptr, *d_roworder = nullptr;
    int *d_cflags = nullptr;     // per instance: KArgs::cflags
    double *d_cache = nullptr;   // solution caches (ACME_SOLVER_CACHING_HOMOTOPY)
    long long *d_report = nullptr;
    double *d_u = nullptr, *d_y = nullptr;  // staging for host-pointer runs
    size_t cap_u = 0, cap_y = 0;
    double *d_uv = nullptr, *d_uc = nullptr; // acme_batch_run_const: the varying rows of a time slice, the rows' constants
    size_t cap_uv = 0, cap_uc = 0;
    be::stream_t copy_stream = nullptr;     // host-pointer runs: copies of slice s+1 / s-1 overlap kernel s
    be::stream_t copy_stream_out = nullptr; // ... the two directions on streams of their own (the bus is full duplex)
    // Host-pointer runs page-lock (register) the caller's u and y for DMA -- copies from pageable memory go through
    // the driver's bounce buffers at less than half the bus rate, and the headline workload moves 11.6 GB in and
    // 2.9 GB out per 0.3 s of kernel time.  Page-locking costs about as much as one copy, so the LAST registered
    // range of each direction is kept: a caller that reuses its arrays across run! calls (what the reference's
    // in-place run!(runner, y, u) is for, src/ACME.jl:650-664) pays once.  Released when another range comes, and
    // by acme_batch_destroy / acme_batch_release_host_buffers.  ACME_HOST_REGISTER=0 keeps the pageable path.
    struct HostReg { const void *ptr = nullptr; size_t bytes = 0; bool ok = false; } reg_u, reg_y;
    // acme_batch_set_host_retention: the caller's u / y arrays may be page-locked and STAY so between runs.  Off by
    // default: a registration that outlives the arrays (a wrapper's per-call temporaries, a garbage-collected array)
    // would hand the copy engine and the kernel pages that no longer exist.
    bool retain_host = false;
    // Isolation of slow instances (acme_batch_set_isolation): the instances that needed more than iso_thr Newton
    // iterations per sample over the previous run are launched on their own, on slow_stream, the others on the caller's
    // stream -- a launch lasts as long as its slowest wave, and a pathological cell of a sweep (e.g. a potentiometer
    // at an end stop that makes the model singular: ~900 iterations per sample where the others need 3) would
    // otherwise hold every other instance's results back by its own, hundreds of times longer, serial recurrence.
    double iso_thr = 0.0;
    be::stream_t slow_stream = nullptr;
    std::vector<int> map_fast, map_slow;     // instance lists of the two groups (empty: one launch over all)
    int *d_map_fast = nullptr, *d_map_slow = nullptr;
    std::vector<long long> iso_iters;        // per instance: iteration total at the last classification
    long long iso_samples = 0;               // samples_done at the last classification
    // Placement of the waves by their measured cost (acme_balance.h, acme_batch_set_balance): -1 = the library decides
    // (on when the launch has more blocks than the chip has compute units), 0 off, 1 on
    int balance = -1;
    int cus = 0;                             // compute units of the batch's device
    bool bal_valid = false;                  // d_map_bal holds a placement ...
    int bal_per = 0;                         // ... of this many instances per wave
    long long bal_samples = 0;               // samples_done at the last balancing
    int *d_map_bal = nullptr;
    long long *d_bal_prev = nullptr;
    unsigned *d_bal_weight = nullptr;
    long long *h_u_ready = nullptr;          // streamed host runs: the copy's progress, in host memory the kernel reads
    const long long *d_u_ready = nullptr;
    acme_progress_fn progress = nullptr;    // @showprogress: called after every time slice of a host-buffer run
    void *progress_user = nullptr;
    // HIP event pairs around the launches, on the launch stream; drained lazily
    static constexpr int NEV = 32;
    be::event_t ev0[NEV] = {}, ev1[NEV] = {};
    int ev_head = 0, ev_pending = 0;
    double ms_sum = 0.0;
    float ms_last = 0.f;
    long long launches = 0;
    long long samples_done = 0;
    size_t lds_bytes = 0;
    long long image_stride = 0;
    int sub_nn[GEN_MAX_SUB] = {}, sub_np[GEN_MAX_SUB] = {};  // actual dims of the sub-problems
    // The model fits none of the tuned kernels' shapes (or ACME_GENERIC=1): the lane-per-instance generic kernel
    // (acme_generic.h) runs it -- any dimensions, any number of sub-problems; never refused
    bool generic = false;
    PackedGeneric G;
    HostModel host_model;                    // the batch model as the caller handed it over (a rebuild needs it)
    bool allow_condense = true;              // false: rebuilt on the plain shape (instances with their own element parameters)
    // condensed shape + per-instance matrices: the models the instances were given (acme_batch_set_matrices), kept until it is
    // clear that no instance needs element parameters of its own -- a rebuild on the plain shape re-applies them
    std::vector<std::unique_ptr<HostModel>> inst_models;
    // per-instance element tables (acme_batch_set_matrices with models whose element PARAMETERS differ): rowc / rowi hold N
    // tables; doubles / ints between them
    long long table_stride = 0, tablei_stride = 0;
    int coop_gpw = 0;          // > 0: run! of this generic batch goes through the cooperative mid-size kernel (acme_coop.h)
    int coop_nc = 0;           // ... in this instantiation (GArgs::coop_nc)
    int coop_wpb = 0, coop_imgl = 0;   // ... in this launch shape (coop_shape: fixed when the batch is created)
    int *d_coop_order = nullptr;       // [N][64]: the row order each instance has learnt (kept between launches)
    GenHeader *d_gh = nullptr;
    double *d_ws = nullptr;
    // Oversampled runs (acme_batch_set_oversampling, acme_resample.h): the model advances k samples per sample of u / y
    struct Oversampling {
        int k = 1;                               // 1: off (none of the members below is used)
        int lu = 0, ld = 0, du = 0;              // tap counts; du = (lu - 1) / k base-rate samples of u history
        unsigned long long held = 0;             // input rows held (zero-order hold)
        bool fresh = true;                       // the next run extends each signal's first sample into the past
        double *d_taps = nullptr;                // k h_up | h_down
        double *d_hist_u = nullptr, *d_hist_y = nullptr;    // [N][du][nu], [N][ld - 1][ny]
        double *d_ou = nullptr, *d_oy = nullptr, *d_base = nullptr;   // a slice at the model rate (u, y); full u rows
        size_t cap_ou = 0, cap_oy = 0, cap_base = 0;
        be::event_t ev[2] = {};                  // host-buffer runs: slice s has been decimated
    } os;
    // Output measurements (acme_batch_set_measurement, acme_measure.h): accumulators per instance and measured row, fed
    // slice by slice from the base-rate outputs of every run while armed (run_os)
    struct Measurement {
        bool on = false;
        long long start = 0, length = 0, f_num = 0, f_den = 1;
        int H = 0, nrows = 0;
        unsigned char row[64] = {};              // the measured rows, ascending
        long long pos = 0;                       // base-rate samples since arming
        double *d_acc = nullptr;                 // [4 + 2H][N nrows]
        double *d_tw = nullptr;                  // one chunk's twiddles, [H][MEAS_CHUNK] pairs
        double *d_ys = nullptr;                  // y = NULL: one slice of base-rate outputs, [N][TS][ny]
        size_t cap_ys = 0;
        // per-instance fundamentals (acme_batch_set_measurement_per_instance): the plan of acme_measure.h, built at arming
        bool pi = false;
        int F = 0;                               // distinct f_num: groups, rows of the table [F][H][chunk]
        long long chunk = MEAS_CHUNK;            // samples per step (the table's budget)
        std::vector<long long> perm;             // the plan on the host (acme_batch_get_measurement_plan)
        std::vector<int> wgrp;
        long long *d_fnum_g = nullptr, *d_perm = nullptr;       // [F], [N nrows]
        int *d_sgrp = nullptr, *d_wgrp = nullptr;               // [N nrows], [(N nrows + 63) / 64]
        // bins (acme_batch_set_measurement_bins): the per-instance plan over groups of distinct tone tuples, H = the bins
        bool bins = false;
        long long *d_kbin_g = nullptr;           // [F][H]: the groups' reduced bin frequencies
        // series (acme_batch_set_measurement_series): W windows of win samples, one every hop; d_acc is [W][4 + 2H][N nrows]
        long long win = 0, hop = 0, W = 0;       // W = 0: one window, [start, start + length)
        // fold (acme_batch_set_measurement_fold): the window folded onto a period per instance, slot m mod period
        bool fold = false;
        long long fold_pmax = 0;                 // the longest period: the accumulators' pitch
        std::vector<long long> fold_per;         // [N]: the instances' periods
        long long *d_fold_per = nullptr;         // [N]
        double *d_fold = nullptr;                // [N nrows][fold_pmax] sums, from 0.0
        // spectrum (acme_batch_set_measurement_spectrum): Welch-averaged periodograms of the window, segments of spec_L
        // samples every spec_hop
        bool spec = false;
        long long spec_L = 0, spec_hop = 0;
        std::vector<double> spec_w, spec_tw;     // [L] the window, [L / 2][2] the twiddles, as the device has them
        double *d_spec_w = nullptr, *d_spec_tw = nullptr;
        double *d_spec_acc = nullptr;            // [N nrows][L / 2 + 1] sums of |X_k|^2, from 0.0
        double *d_spec_carry = nullptr;          // [N nrows][L]: the window's most recent samples, sample m at m mod L
        // cross-spectrum (acme_batch_set_measurement_cross): the spectrum's segments of input row cross_in and the measured
        // rows, packed into one complex transform per pair
        bool cross = false;
        int cross_in = 0;
        long long cross_L = 0, cross_hop = 0;
        std::vector<double> cross_w, cross_tw;   // [L] the window, [L / 2][2] the twiddles, as the device has them
        double *d_cross_w = nullptr, *d_cross_tw = nullptr;
        double *d_cross_acc = nullptr;           // [N nrows][4][L / 2 + 1] sums of |X|^2, |Y|^2, Re and Im conj(X) Y, from 0.0
        double *d_cross_carry = nullptr;         // [N nrows][2][L]: the most recent samples of x and of y, sample m at m mod L
        // target (acme_batch_set_measurement_target): the residual against a looped waveform of the caller's
        bool target = false;
        long long tgt_K = 0, tgt_P = 0;
        double tgt_c = 0.0;                      // the pre-emphasis coefficient
        double *d_tgt = nullptr;                 // [K][nrows][P]
        int *d_tgt_which = nullptr, *d_tgt_wuni = nullptr;      // [N], [(N nrows + 63) / 64]: the plan (meas_target_plan)
        long long *d_tgt_lag = nullptr;          // [N]
        double *d_tgt_acc = nullptr;             // [9][N nrows]: the seven chains and the carries e_prev, t_prev, from 0.0
        // ensemble (acme_batch_set_measurement_ensemble): per-sample statistics across the instances of a group
        bool ens = false;
        int ens_G = 0;
        long long ens_stride = 0, ens_E = 0;     // E = ceil(length / stride) slots
        std::vector<long long> ens_off;          // [G + 1]: the plan's offsets on the host (the getter's members)
        int *d_ens_member = nullptr;             // the plan (meas_ensemble_plan): instances sorted by (group, instance)
        long long *d_ens_off = nullptr;          // [G + 1]
        double *d_ens_acc = nullptr;             // [6][G nrows][E]: S, Q, min, max, then imin, imax as long long
        // histogram (acme_batch_set_measurement_histogram): the amplitude distribution of every (instance, row) pair
        bool hist = false;
        int hist_B = 0, hist_mode = 0;
        std::vector<double> hist_range;          // [N][3]: lo_i, hi_i, s_i on the host (the getter's range)
        long long *d_hist_cnt = nullptr;         // [N nrows][B + 3]: UNDER, BIN[0 ... B - 1], OVER, NAN, from 0
        double *d_hist_range = nullptr;          // [N][3]
        // events (acme_batch_set_measurement_events): level crossings of every (instance, row, level) triple
        bool events = false;
        int ev_C = 0, ev_E = 0;
        std::vector<double> ev_lev;              // [2][C][N]: lo, then hi, on the host
        double *d_ev_lev = nullptr;              // [2][C][N]
        long long *d_ev_cnt = nullptr;           // [N nrows C][5]: RISE, FALL, HIGH, LOW, UNKNOWN
        long long *d_ev_idx = nullptr;           // [N nrows C][2][E + 1]: the events' window samples, -1: empty
        double *d_ev_ab = nullptr;               // [N nrows C][2][E + 1][2]: v[m - 1], v[m]
        int *d_ev_state = nullptr;               // the carry: [N nrows C] states ...
        double *d_ev_prev = nullptr;             // ... and [N nrows] last window samples
        // weighting (acme_batch_set_measurement_weighting): a biquad cascade ahead of every form; wS = 0: none
        int wS = 0;
        double wsos[MEAS_MAX_WEIGHT_SECTIONS][5] = {};          // b0 b1 b2 a1 a2
        double *d_wstate = nullptr;              // [2 wS][N nrows]: the sections' s1 and s2, from 0.0
        double *d_yw = nullptr;                  // one slice of weighted rows, [N][n][nrows] (grow-only)
        size_t cap_yw = 0;
    } meas;
    // Input rows generated on the device (acme_batch_set_source_*, acme_source.h): the rows' descriptions and per-instance
    // parameters in device memory, the source clock
    struct Sources {
        int armed = 0;                           // rows with a source (0: none of the members below is used)
        unsigned long long mask = 0, cmask = 0;  // the rows with a source; those of kind CONST (held on an oversampled batch)
        long long clock = 0;                     // base-rate samples since the first source was armed
        SrcRow row[64] = {};                     // as the device sees them (the pointers are device pointers)
        SrcRow *d_rows = nullptr;                // [64]
        double *d_ys = nullptr;                  // device arrays, y stored, no oversampling: one slice of packed outputs
        size_t cap_ys = 0;
    } src;
    // acme_batch_run_async: the run in flight on a worker thread of the library, its status and message
    std::thread worker;
    int worker_rc = ACME_OK;
    std::string worker_err;
};

// Every entry point that takes a batch first joins an asynchronous run that is still in flight
// (acme_batch_run_async): the handle stays single-owner, nothing ever sees a half-advanced batch.
// The run's own status is kept for acme_batch_wait.
static void join_worker(acme_batch *b) {
    if (b && b->worker.joinable()) b->worker.join();
}
// The prologue of everything that runs a batch: join its worker (NULL: the caller is the worker), then hold the backend's
// run mutex, if it has one, to the end of the call -- the CPU emulator backend is not re-entrant, and a worker of
// ANOTHER batch may be running.
struct RunGuard {
    std::unique_lock<std::mutex> serial;
    explicit RunGuard(acme_batch *join) {
        join_worker(join);
        if (std::mutex *m = be::run_mutex()) serial = std::unique_lock<std::mutex>(*m);
    }
};
// start `run` (-> status) on the batch's worker thread (acme_batch_run_async; the worker has been joined)
template <class Run>
static int start_worker(acme_batch *b, Run run) {
    if (b->worker_rc != ACME_OK) {       // a failed asynchronous run nobody waited for: reported now, not dropped
        const int rc = b->worker_rc;
        b->worker_rc = ACME_OK;
        return fail(rc, "previous asynchronous run failed: " + b->worker_err);
    }
    b->worker_err.clear();
    try {
        b->worker = std::thread([b, run]() {
            RunGuard serial(nullptr);    // (the synchronous entry points join b->worker first: not from the worker itself)
            b->worker_rc = run();
            if (b->worker_rc != ACME_OK) b->worker_err = g_err;      // the worker's thread-local message
        });
    } catch (const std::exception &e) {
        return fail(ACME_ERR_HIP, std::string("cannot start the worker thread: ") + e.what());
    }
    return ACME_OK;
}

// free the per-instance parameters of input row `row`'s source (row < 0: of every row) and mark the row as the caller's
static void src_release(acme_batch *b, int row) {
    acme_batch::Sources &S = b->src;
    for (int r = row < 0 ? 0 : row; r < (row < 0 ? 64 : row + 1); ++r) {
        SrcRow &R = S.row[r];
        if (R.kind == SRC_NONE) continue;
        (void)be::dfree(const_cast<double *>(R.amp)); (void)be::dfree(const_cast<double *>(R.off)); (void)be::dfree(const_cast<double *>(R.w));
        (void)be::dfree(const_cast<long long *>(R.fnum)); (void)be::dfree(const_cast<long long *>(R.phase));
        (void)be::dfree(const_cast<long long *>(R.shape));
        R = SrcRow{};
        S.mask &= ~(1ull << r);
        S.cmask &= ~(1ull << r);
        --S.armed;
    }
}

static void release_reg(acme_batch::HostReg &r) {
    if (r.ok) (void)be::host_unregister(const_cast<void *>(r.ptr));
    r = acme_batch::HostReg{};
}
// page-lock [p, p + bytes) unless it already is; false: the run proceeds from pageable memory
static bool ensure_registered(acme_batch::HostReg &r, const void *p, size_t bytes) {
    const char *e = getenv("ACME_HOST_REGISTER");
    size_t least = (size_t)1 << 20;                                                // (small runs: not worth a system call)
    if (const char *m = getenv("ACME_HOST_REGISTER_MIN")) least = (size_t)atoll(m);     // (tests)
    if ((e && e[0] == '0') || !p || bytes < least) return false;
    if (r.ok && r.ptr == p && r.bytes >= bytes) return true;
    release_reg(r);
    if (be::host_register(const_cast<void *>(p), bytes) != 0) return false;      // (e.g. memory that cannot be locked)
    r.ptr = p; r.bytes = bytes; r.ok = true;
    return true;
}

static void fill_args(const acme_batch *b, KArgs &A) {
    A.image = b->d_image;
    A.image_stride = b->image_stride;
    A.rowc = b->d_rowc;
    A.rowi = b->d_rowi;
    A.table_stride = b->table_stride;
    A.tablei_stride = b->tablei_stride;
    A.lanec = b->d_lanec;
    A.state = b->d_state;
    A.report = b->d_report;
    A.roworder = b->d_roworder;
    A.cache = b->d_cache;
    A.n_inst = b->N;
    A.sample_base = b->samples_done;
    A.tol = b->o.tol;
    A.maxiter = b->o.maxiter;
    A.solver = b->o.solver;
    A.nu_io = b->P.actual.nu;
    A.ny_io = b->P.actual.ny;
    A.nterms = b->P.nterms;
    A.has_bjt = b->P.has_bjt;
    A.rare_kinds = b->P.rare_kinds;
    A.nsub = b->P.actual.nsub;
    for (int i = 0; i < GROUP; ++i) A.zperm[i] = b->P.zperm[i];
    A.cflags = b->d_cflags;
}

// run! goes through the lane-per-instance kernel (acme_lane_kernel.h) when the model is small enough
// for it: one shared image, one nonlinear sub-problem of unified element rows, a shape it is built
// for.  ACME_LANE_KERNEL=0 in the environment keeps the 16-lane kernel (A/B measurements, tests).
static bool use_lane_kernel(const acme_batch *b) {
    if (b->generic) return false;
    if (!b->k->launch_lane || !b->k->lds_lane_plain || !b->d_lanec) return false;
    if (b->image_stride != 0 || b->P.actual.nsub != 1 || b->P.rare_kinds || b->low) return false;
    const char *e = getenv("ACME_LANE_KERNEL");
    return !(e && e[0] == '0');
}
static size_t lane_lds_bytes(const acme_batch *b) {
    return sizeof(double) * (size_t)(b->o.solver == ACME_SOLVER_CACHING_HOMOTOPY ? b->k->lds_lane_caching : b->k->lds_lane_plain);
}

// retire the `count` oldest recorded event pairs into the kernel-time statistics
static int drain_events(acme_batch *b, int count) {
    for (int i = 0; i < count && b->ev_pending > 0; ++i) {
        const int slot = b->ev_head;
        HIPCHK(be::event_sync(b->ev1[slot]));
        float ms = 0.f;
        HIPCHK(be::event_elapsed(&ms, b->ev0[slot], b->ev1[slot]));
        b->ms_last = ms;
        b->ms_sum += ms;
        ++b->launches;
        b->ev_head = (b->ev_head + 1) % acme_batch::NEV;
        --b->ev_pending;
    }
    return ACME_OK;
}

extern "C" {

const char *acme_last_error(void) { return g_err.c_str(); }

int acme_device_count(void) {
    int n = 0;
    if (be::device_count(&n) != 0) return 0;
    return n;
}

void acme_default_options(acme_options *o) {
    if (!o) return;
    o->solver = ACME_SOLVER_HOMOTOPY;
    o->tol = 1e-10;
    o->maxiter = 500;
    o->device = -1;
    o->per_instance_matrices = 0;
}

static void copyv(std::vector<double> &dst, const double *src, size_t n) {
    dst.assign(n, 0.0);
    if (src && n) memcpy(dst.data(), src, n * sizeof(double));
}

int acme_model_create(int nx, int nu, int ny, int nn_total, const double *a, const double *b, const double *c,
                      const double *x0, const double *dy, const double *ey, const double *fy, const double *y0,
                      acme_model **out) {
    if (!out || nx < 0 || nu < 0 || ny < 0 || nn_total < 0) return fail(ACME_ERR_INVALID, "invalid model dimensions");
    auto *m = new acme_model();
    m->h.nx = nx; m->h.nu = nu; m->h.ny = ny; m->h.nn_total = nn_total;
    copyv(m->h.a, a, (size_t)nx * nx);
    copyv(m->h.b, b, (size_t)nx * nu);
    copyv(m->h.c, c, (size_t)nx * nn_total);
    copyv(m->h.x0, x0, nx);
    copyv(m->h.dy, dy, (size_t)ny * nx);
    copyv(m->h.ey, ey, (size_t)ny * nu);
    copyv(m->h.fy, fy, (size_t)ny * nn_total);
    copyv(m->h.y0, y0, ny);
    *out = m;
    return ACME_OK;
}

int acme_model_add_subproblem(acme_model *m, int nn, int nq, int np, const double *pexp, const double *dq,
                              const double *eq, const double *fqprev, const double *fq, const double *q0,
                              const double *init_z, int n_elems, const int *elem_kind, const int *elem_qoff,
                              const int *elem_roff, const double *elem_par) {
    if (!m || nn < 0 || nq < 0 || np < 0 || n_elems < 0) return fail(ACME_ERR_INVALID, "invalid sub-problem");
    HostSub s;
    s.nn = nn; s.nq = nq; s.np = np;
    copyv(s.pexp, pexp, (size_t)nq * np);
    copyv(s.dq, dq, (size_t)np * m->h.nx);
    copyv(s.eq, eq, (size_t)np * m->h.nu);
    copyv(s.fqprev, fqprev, (size_t)np * m->h.nn_total);
    copyv(s.fq, fq, (size_t)nq * nn);
    copyv(s.q0, q0, nq);
    copyv(s.init_z, init_z, nn);
    for (int e = 0; e < n_elems; ++e) {       // what the element table can hold (include/acme_hip.h: ACME_KIND_*)
        if (elem_kind[e] < ACME_KIND_DIODE || elem_kind[e] > ACME_KIND_JA)
            return fail(ACME_ERR_INVALID, "unknown element kind " + std::to_string(elem_kind[e]));
        if (elem_kind[e] == ACME_KIND_MOSFET) {
            const double *p = elem_par + (size_t)e * MAX_ELEM_PAR;
            if (!(p[2] >= 1 && p[2] <= 4 && p[7] >= 1 && p[7] <= 4 && p[2] == (int)p[2] && p[7] == (int)p[7]))
                return fail(ACME_ERR_UNSUPPORTED, "MOSFET threshold / gain polynomials (vt, alpha; src/elements.jl:436-450) are limited to "
                                                  "1 ... 4 coefficients each by the element table's 16 parameters per element");
        }
    }
    s.kind.assign(elem_kind, elem_kind + n_elems);
    s.qoff.assign(elem_qoff, elem_qoff + n_elems);
    s.roff.assign(elem_roff, elem_roff + n_elems);
    copyv(s.par, elem_par, (size_t)n_elems * MAX_ELEM_PAR);
    m->h.subs.push_back(std::move(s));
    return (int)m->h.subs.size() - 1;
}

int acme_model_set_row_order(acme_model *m, int sub, const int *order, int n) {
    if (!m || sub < 0 || sub >= (int)m->h.subs.size() || n < 0 || (n > 0 && !order))
        return fail(ACME_ERR_INVALID, "invalid argument to acme_model_set_row_order");
    if (n != 0 && n != m->h.subs[sub].nn) return fail(ACME_ERR_INVALID, "row order must have nn entries");
    m->h.subs[sub].row_order.assign(order, order + n);
    return ACME_OK;
}

void acme_model_destroy(acme_model *m) { delete m; }

int acme_model_kernel_shape(const acme_model *m, int dims[6]) {
    if (!m || !dims) return fail(ACME_ERR_INVALID, "null argument");
    Packed P;
    std::string err;
    if (!pack_model(m->h, P, err)) {      // the generic kernel takes it as it is: the model's own (largest) dimensions
        PackedGeneric G;
        if (!pack_generic(m->h, G, err)) return fail(ACME_ERR_UNSUPPORTED, err);
        dims[0] = G.H.nnmax; dims[1] = G.H.nqmax; dims[2] = G.H.npmax;
        dims[3] = G.H.nx; dims[4] = G.H.nu; dims[5] = G.H.ny;
        return ACME_OK;
    }
    dims[0] = P.shape.nn; dims[1] = P.shape.nq; dims[2] = P.shape.np;
    dims[3] = P.shape.nx; dims[4] = P.shape.nu; dims[5] = P.shape.ny;
    return ACME_OK;
}

// Which instantiation of the cooperative kernel runs a model (GArgs::coop_nc).  ONE sub-problem of 17 ... 32 unknowns: the
// Jacobian's rows in registers, NC = the unknowns rounded up to four columns, eliminated in a learnt row order with
// threshold pivoting (acme_coop.h "the THRESHOLD path").  Any other single sub-problem of up to 64 unknowns: the same
// elimination on one matrix in LDS, -NS with NS = the rows per lane in use.  0 -- no sub-problem at all, or
// ACME_COOP_LITERAL=1 in the environment when the batch is created (A/B measurements, tests): the any-size instantiation,
// the reference's pivoting literally with everything in LDS.  ACME_COOP_REG=0: no register instantiations (their sizes
// take the matrix-in-LDS ones).
static int coop_register_columns(const GenHeader &H) {
    const char *e = getenv("ACME_COOP_REG"), *lit = getenv("ACME_COOP_LITERAL");
    if (lit && lit[0] == '1') return 0;
    if (H.nsub != 1 || H.sub[0].nn < 1 || H.sub[0].nn > COOP_MAX_N) return 0;
    const int nn = H.sub[0].nn;
    if (!(e && e[0] == '0') && nn > GROUP && nn <= GROUP * COOP_REG_SLOTS) return (nn + 3) & ~3;
    // matrix in LDS: beyond 32 unknowns one instance per wave, one row per lane (ACME_COOP_WAVE64=1: whatever the size; =0:
    // never -- one instance per 16 lanes with several rows per lane, for A/B measurements)
    const char *w = getenv("ACME_COOP_WAVE64");
    if (w ? w[0] == '1' : nn > GROUP * COOP_REG_SLOTS) return COOP_WAVE64;
    return -((nn + GROUP - 1) / GROUP);
}
// LDS of one block: [ image (staged only if shared by the batch) | row tables | wpb x gpw x (workspace | cache p's) ]
static size_t coop_lds_bytes(const GenHeader &H, bool image_in_lds, int wpb, int gpw, int nc) {
    size_t pad = 0;
    if (const char *e = getenv("ACME_COOP_LDS_PAD")) pad = (size_t)atoll(e);          // (developer: bytes of slack behind the block's LDS)
    return sizeof(double) * ((size_t)coop_shared_doubles(H, image_in_lds, nc) + (size_t)wpb * (size_t)gpw * (size_t)coop_inst_doubles(H, nc)) + pad;
}
// The mid-size kernel (acme_coop.h) takes a model the tuned shapes do not hold when it has at most ONE nonlinear
// sub-problem of up to 64 unknowns / parameters and an instance's working arrays fit the LDS of a compute unit.  Its launch
// shape -- waves per block (they share the row tables and the staged image), instances per wave, image in LDS or in L2 --
// is whatever keeps most instances resident per compute unit (the kernel is bound by one wave's instruction issue and
// latencies: more resident instances is the one thing that always pays); among equals the image in LDS (evaluate!, the
// closures and the state update read it with dependent loads), then full waves.  The instantiations with the factorisation
// in registers take more than 256 registers: one wave per SIMD, four per compute unit.  gpw == 0: the lane-per-instance
// generic kernel has to take the model.  ACME_COOP=0 in the environment: never; ACME_COOP_GPW / ACME_COOP_WPB /
// ACME_COOP_IMGL pin a choice (A/B measurements, tests; ignored where they do not fit).
struct CoopShape { int wpb = 0, gpw = 0, imgl = 0; long long resident = 0; };          // (resident: instances per compute unit)
static CoopShape coop_shape(const GenHeader &H, int nc, bool shared_image) {
    CoopShape best;
    const char *e = getenv("ACME_COOP");
    if (e && e[0] == '0') return best;
    if (H.nsub > 1 || H.nnmax > COOP_MAX_N || H.npmax > COOP_MAX_N || H.nu > COOP_MAX_N) return best;
    auto pinned = [](const char *name) { const char *v = getenv(name); return v && v[0] >= '0' && v[0] <= '9' ? v[0] - '0' : -1; };
    const int pin_g = pinned("ACME_COOP_GPW"), pin_w = pinned("ACME_COOP_WPB"), pin_i = pinned("ACME_COOP_IMGL");
    const size_t cu = 160u * 1024u;
    const int max_waves = nc > 0 ? 4 : 8;          // (register instantiations: one wave per SIMD; the others are held to 256 registers)
    for (int pass = 0; pass < 2 && best.gpw == 0; ++pass) {          // (second pass: the pins that fit nothing are dropped)
        long long best_score = -1;
        for (int wpb = 4; wpb >= 1; --wpb)
            for (int gpw = nc == COOP_WAVE64 ? 1 : 4; gpw >= 1; gpw /= 2)
                for (int imgl = shared_image ? 1 : 0; imgl >= 0; --imgl) {
                    if (pass == 0 && ((pin_g > 0 && gpw != pin_g) || (pin_w > 0 && wpb != pin_w) || (pin_i >= 0 && imgl != pin_i))) continue;
                    const size_t lds = coop_lds_bytes(H, imgl != 0, wpb, gpw, nc);
                    if (lds > cu) continue;
                    size_t blocks = cu / lds;
                    if (blocks * wpb > (size_t)max_waves) blocks = max_waves / wpb;
                    if (blocks == 0) continue;
                    const long long score = (long long)(blocks * wpb * gpw) * 1000 + imgl * 100 + gpw * 10 + wpb;
                    if (score > best_score) { best_score = score; best.wpb = wpb; best.gpw = gpw; best.imgl = imgl; best.resident = (long long)(blocks * wpb * gpw); }
                }
    }
    return best;
}

// the row order the instances of a mid-size batch start from: every row in its own place.  (ACME_COOP_ORDER=reversed in the
// environment, tests: position p starts with row nn - 1 - p -- an order the first elimination cannot keep, so that the
// re-learning path runs at once.)
static std::vector<int> coop_initial_order(const GenHeader &H, size_t n) {
    std::vector<int> ord(n * COOP_MAX_N);
    const char *e = getenv("ACME_COOP_ORDER");
    const int nn = H.nsub == 1 ? H.sub[0].nn : 0;
    const bool rev = e && e[0] == 'r';
    for (size_t k = 0; k < ord.size(); ++k) {
        const int p = (int)(k % COOP_MAX_N);
        ord[k] = rev && p < nn ? nn - 1 - p : p;
    }
    return ord;
}

static void fill_coop(const acme_batch *b, GArgs &A) {
    A.coop_wpb = b->coop_wpb;
    A.coop_gpw = b->coop_gpw;
    A.coop_imgl = b->coop_imgl;
    A.coop_nc = b->coop_nc;
    A.coop_order = b->d_coop_order;
}

int acme_model_kernel_variant(const acme_model *m, int *condensed_rows, int *generic) {
    if (!m) return fail(ACME_ERR_INVALID, "null argument");
    Packed P;
    std::string err;
    const bool tuned = pack_model(m->h, P, err);
    int gen = 0;
    if (!tuned) {
        PackedGeneric G;
        if (!pack_generic(m->h, G, err)) return fail(ACME_ERR_UNSUPPORTED, err);
        G.H.jp_sparse = G.H.ell;          // (as a batch sharing the model's image would run it)
        gen = coop_shape(G.H, coop_register_columns(G.H), true).gpw > 0 ? 2 : 1;
    }
    if (condensed_rows) *condensed_rows = tuned ? P.shape.nl : 0;
    if (generic) *generic = gen;
    return ACME_OK;
}

// A fresh CachingSolver holds one stored solution, its initial point (p = 0, z = init_z)
// (src/solvers.jl:327-333).  HBM layout per sub-problem: cp[np][CACHE] | count, head | cz[CACHE][nn]
static void fresh_cache(const acme_batch *b, const Packed &P, double *dst) {
    const Dims &S = b->k->d;
    const int nsub = S.nsub > 0 ? S.nsub : 1;
    const int c1 = (S.np + S.nn) * CACHE + 2;
    for (int i = 0; i < nsub * c1; ++i) dst[i] = 0.0;
    for (int s = 0; s < nsub; ++s) {
        double *cz = dst + s * c1 + S.np * CACHE + 2;
        for (int i = 0; i < S.nn; ++i) cz[i] = P.init_state[(size_t)S.nx + (size_t)nsub * S.np + (size_t)s * S.nn + i];
        int meta[2] = {1, 0};
        memcpy(dst + s * c1 + S.np * CACHE, meta, sizeof meta);
    }
}
static void fresh_cache_generic(const PackedGeneric &G, double *dst) {
    const GenHeader &H = G.H;
    for (int i = 0; i < H.cache_total; ++i) dst[i] = 0.0;
    for (int s = 0; s < H.nsub; ++s) {
        const GenSub &g = H.sub[s];
        double *cz = dst + g.c_off + g.np * CACHE + 2;
        for (int i = 0; i < g.nn; ++i) cz[i] = G.init_state[(size_t)H.nx + H.npt + g.zoff + i];
        int meta[2] = {1, 0};
        memcpy(dst + g.c_off + g.np * CACHE, meta, sizeof meta);
    }
}
static int state_doubles(const acme_batch *b) { return b->generic ? b->G.H.state_total : b->k->state; }
static int cache_doubles(const acme_batch *b) {        // per instance, in HBM
    if (b->generic) return b->G.H.cache_total;
    const Dims &S = b->k->d;
    return (S.nsub > 0 ? S.nsub : 1) * ((S.np + S.nn) * CACHE + 2);
}
static int cache_lds_doubles(const acme_batch *b) { return b->k->cache_lds; }   // per instance, in LDS (Shape::CACHEI)

static int init_state(acme_batch *b) {
    const int S = state_doubles(b);
    std::vector<double> st((size_t)b->N * S);
    const double *init = b->generic ? b->G.init_state.data() : b->P.init_state.data();
    for (long long i = 0; i < b->N; ++i) memcpy(&st[(size_t)i * S], init, S * sizeof(double));
    if (S) HIPCHK(be::copy_h2d(b->d_state, st.data(), st.size() * sizeof(double)));
    {
        const int cd = cache_doubles(b);
        std::vector<double> one(cd), all((size_t)b->N * cd);
        if (b->generic) fresh_cache_generic(b->G, one.data());
        else fresh_cache(b, b->P, one.data());
        for (long long i = 0; i < b->N; ++i) memcpy(&all[(size_t)i * cd], one.data(), cd * sizeof(double));
        HIPCHK(be::copy_h2d(b->d_cache, all.data(), all.size() * sizeof(double)));
    }
    return acme_batch_reset_report(b);
}

static int create_batch(const HostModel &hm, long long n, const acme_options *opts, bool allow_condense, acme_batch **out);
int acme_batch_create(const acme_model *m, long long n, const acme_options *opts, acme_batch **out) {
    if (!m || !out || n <= 0) return fail(ACME_ERR_INVALID, "invalid argument to acme_batch_create");
    return create_batch(m->h, n, opts, true, out);
}
}  // extern "C"

static int create_batch(const HostModel &hm, long long n, const acme_options *opts, bool allow_condense, acme_batch **out) {
    struct ModelView { const HostModel &h; } mv{hm};
    const ModelView *m = &mv;
    int ndev = acme_device_count();
    if (ndev <= 0) return fail(ACME_ERR_NO_DEVICE, "no HIP device available; acme_hip has no CPU fallback");
    // any failure below releases what has been allocated so far (acme_batch_destroy copes with a
    // partially built batch)
    struct Destroy { void operator()(acme_batch *p) const { acme_batch_destroy(p); } };
    std::unique_ptr<acme_batch, Destroy> b(new acme_batch());
    if (opts) b->o = *opts; else acme_default_options(&b->o);
    if (b->o.solver != ACME_SOLVER_SIMPLE && b->o.solver != ACME_SOLVER_HOMOTOPY &&
        b->o.solver != ACME_SOLVER_CACHING_HOMOTOPY)
        return fail(ACME_ERR_INVALID, "unknown solver");
    HIPCHK(be::get_device(&b->device));       // device = -1: the caller's current device
    if (b->o.device >= 0) {
        if (b->o.device >= ndev) return fail(ACME_ERR_INVALID, "device ordinal out of range");
        b->device = b->o.device;
    }
    ON_DEVICE(b);
    std::string err;
    {
        const char *fg = getenv("ACME_GENERIC");
        const bool force = fg && fg[0] == '1';
        b->host_model = hm;
        b->allow_condense = allow_condense;
        if (force || !pack_model(m->h, b->P, err, nullptr, nullptr, allow_condense)) {
            std::string err2;
            if (!pack_generic(m->h, b->G, err2)) return fail(ACME_ERR_UNSUPPORTED, force ? err2 : err + "; " + err2);
            b->generic = true;
        }
    }
    for (size_t k = 0; k < m->h.subs.size() && k < (size_t)GEN_MAX_SUB; ++k) {
        b->sub_nn[k] = m->h.subs[k].nn;
        b->sub_np[k] = m->h.subs[k].np;
    }
    if (b->generic) {
        b->G.H.jp_sparse = b->G.H.ell && b->o.per_instance_matrices == 0;
        const GenHeader &H = b->G.H;
        b->coop_nc = coop_register_columns(H);
        {
            // the launch shape is decided HERE, once (the environment is not consulted again: ADVICE r5), and the
            // instantiation's LDS is asked for on the batch's device
            CoopShape cs = coop_shape(H, b->coop_nc, b->o.per_instance_matrices == 0);
            if (b->coop_nc > 0 && H.ell && b->o.per_instance_matrices == 0) {
                // register instantiations: the matrices' sparse forms staged beside the dense ones (ACME_COOP_REG_SPARSE=0: never)
                // where that keeps as many instances resident and the image in LDS
                const char *e = getenv("ACME_COOP_REG_SPARSE");
                b->G.H.reg_sparse = 1;
                const CoopShape cs1 = coop_shape(b->G.H, b->coop_nc, true);
                if (!(e && e[0] == '0') && cs1.gpw > 0 && cs1.resident >= cs.resident && cs1.imgl >= cs.imgl) cs = cs1;
                else b->G.H.reg_sparse = 0;
            }
            b->coop_gpw = cs.gpw;
            b->coop_wpb = cs.wpb;
            b->coop_imgl = cs.imgl;
        }
        b->P = Packed{};
        b->P.actual = Dims{H.nnmax, H.nqmax, H.npmax, H.nx, H.nu, H.ny, 0, H.nsub, 0};
        b->P.shape = b->P.actual;
        for (int i = 0; i < GROUP; ++i) b->P.zperm[i] = b->P.zinv[i] = i;
        b->N = n;
        const bool per = b->o.per_instance_matrices != 0;
        const size_t img = b->G.image.size();
        b->image_stride = per ? (long long)img : 0;
        HIPCHK(be::dmalloc((void **)&b->d_image, sizeof(double) * img * (per ? (size_t)n : 1)));
        for (long long i = 0; i < (per ? n : 1); ++i)
            HIPCHK(be::copy_h2d(b->d_image + (size_t)i * img, b->G.image.data(), img * sizeof(double)));
        HIPCHK(be::dmalloc((void **)&b->d_rowc, sizeof(double) * b->G.rowc.size()));
        HIPCHK(be::copy_h2d(b->d_rowc, b->G.rowc.data(), sizeof(double) * b->G.rowc.size()));
        HIPCHK(be::dmalloc((void **)&b->d_rowi, sizeof(int) * b->G.rowi.size()));
        HIPCHK(be::copy_h2d(b->d_rowi, b->G.rowi.data(), sizeof(int) * b->G.rowi.size()));
        HIPCHK(be::dmalloc((void **)&b->d_gh, sizeof(GenHeader)));
        HIPCHK(be::copy_h2d(b->d_gh, &b->G.H, sizeof(GenHeader)));
        HIPCHK(be::dmalloc((void **)&b->d_ws, sizeof(double) * (size_t)n * H.ws_total));
        if (b->coop_gpw > 0) {
            const std::vector<int> ord = coop_initial_order(H, (size_t)n);
            HIPCHK(be::dmalloc((void **)&b->d_coop_order, sizeof(int) * ord.size()));
            HIPCHK(be::copy_h2d(b->d_coop_order, ord.data(), sizeof(int) * ord.size()));
            GArgs A{};
            fill_coop(b.get(), A);
            HIPCHK(be::coop_prepare(A, coop_lds_bytes(H, b->coop_imgl != 0, b->coop_wpb, b->coop_gpw, b->coop_nc)));
        }
        HIPCHK(be::dmalloc((void **)&b->d_state, sizeof(double) * (size_t)n * (H.state_total ? H.state_total : 1)));
        HIPCHK(be::dmalloc((void **)&b->d_report, sizeof(long long) * (size_t)n * RW_WORDS));
        HIPCHK(be::dmalloc((void **)&b->d_cache, sizeof(double) * (size_t)n * H.cache_total));
        {
            std::vector<int> cf((size_t)n, 1);
            HIPCHK(be::dmalloc((void **)&b->d_cflags, sizeof(int) * cf.size()));
            HIPCHK(be::copy_h2d(b->d_cflags, cf.data(), sizeof(int) * cf.size()));
        }
        for (int i = 0; i < acme_batch::NEV; ++i) {
            HIPCHK(be::event_create(&b->ev0[i]));
            HIPCHK(be::event_create(&b->ev1[i]));
        }
        int rc = init_state(b.get());
        if (rc != ACME_OK) return rc;
        *out = b.release();
        return ACME_OK;
    }
    b->k = find_kernel(b->P.shape);
    if (!b->k) return fail(ACME_ERR_UNSUPPORTED, "kernel shape not instantiated");
    b->N = n;
    const bool per = b->o.per_instance_matrices != 0;
    const size_t img = b->P.image.size();
    b->image_stride = per ? (long long)img : 0;
    const size_t cache_lds = b->o.solver == ACME_SOLVER_CACHING_HOMOTOPY ? (size_t)INST_PER_BLOCK * cache_lds_doubles(b.get()) : 0;
    b->lds_bytes = sizeof(double) * ((size_t)(per ? b->k->lds_per_inst : b->k->lds_shared) + cache_lds);
    b->kf = &b->k->lds;
    // The image(s) -- 16 private ones per block, or the shared one next to the solution caches -- do not
    // fit the 160 KiB of a CU: the LOW-LDS kernels read them from HBM / L2 instead (slower; never refused).
    // ACME_LOW_LDS=1 in the environment forces that variant where it exists (tests, A/B measurements).
    const char *force_low = getenv("ACME_LOW_LDS");
    if (b->lds_bytes > 160 * 1024 || (force_low && force_low[0] == '1' && b->k->low.fn)) {
        if (!b->k->low.fn) return fail(ACME_ERR_UNSUPPORTED, "model does not fit the LDS of a CU and its shape has no LOW-LDS kernel");
        b->low = true;
        b->kf = &b->k->low;
        b->lds_bytes = sizeof(double) * ((size_t)b->k->lds_low + cache_lds);
    }
    HIPCHK(be::set_max_lds(b->kf->fn, (int)b->lds_bytes));
    if (b->kf->fn_jac) HIPCHK(be::set_max_lds(b->kf->fn_jac, (int)b->lds_bytes));
    if (b->kf->fn_solve) HIPCHK(be::set_max_lds(b->kf->fn_solve, (int)b->lds_bytes));
    if (b->kf->fn_stream) HIPCHK(be::set_max_lds(b->kf->fn_stream, (int)b->lds_bytes));
    if (b->k->fn_lane && b->k->lds_lane_plain) HIPCHK(be::set_max_lds(b->k->fn_lane, (int)lane_lds_bytes(b.get())));
    HIPCHK(be::dmalloc((void **)&b->d_image, sizeof(double) * img * (per ? (size_t)n : 1)));
    if (per) {
        std::vector<double> all(img * (size_t)n);
        for (long long i = 0; i < n; ++i) memcpy(&all[(size_t)i * img], b->P.image.data(), img * sizeof(double));
        HIPCHK(be::copy_h2d(b->d_image, all.data(), all.size() * sizeof(double)));
    } else {
        HIPCHK(be::copy_h2d(b->d_image, b->P.image.data(), img * sizeof(double)));
    }
    HIPCHK(be::dmalloc((void **)&b->d_rowc, sizeof(double) * b->P.rowc.size()));
    HIPCHK(be::copy_h2d(b->d_rowc, b->P.rowc.data(), sizeof(double) * b->P.rowc.size()));
    if (!b->P.lanec.empty()) {
        HIPCHK(be::dmalloc((void **)&b->d_lanec, sizeof(double) * b->P.lanec.size()));
        HIPCHK(be::copy_h2d(b->d_lanec, b->P.lanec.data(), sizeof(double) * b->P.lanec.size()));
    }
    HIPCHK(be::dmalloc((void **)&b->d_rowi, sizeof(int) * b->P.rowi.size()));
    HIPCHK(be::copy_h2d(b->d_rowi, b->P.rowi.data(), sizeof(int) * b->P.rowi.size()));
    HIPCHK(be::dmalloc((void **)&b->d_state, sizeof(double) * (size_t)n * (b->k->state ? b->k->state : 1)));
    HIPCHK(be::dmalloc((void **)&b->d_report, sizeof(long long) * (size_t)n * RW_WORDS));
    HIPCHK(be::dmalloc((void **)&b->d_cache, sizeof(double) * (size_t)n * cache_doubles(b.get())));
    {
        const int nsub_shape = b->k->d.nsub > 0 ? b->k->d.nsub : 1;
        std::vector<int> ro((size_t)n * nsub_shape * GROUP);
        for (size_t i = 0; i < ro.size(); ++i) ro[i] = (int)(i % GROUP);
        HIPCHK(be::dmalloc((void **)&b->d_roworder, sizeof(int) * ro.size()));
        HIPCHK(be::copy_h2d(b->d_roworder, ro.data(), sizeof(int) * ro.size()));
        // (a freshly constructed solver's origin is (0, init_z): on the linear rows only to the tolerance of the
        // front end's initial solve)
        std::vector<int> cf((size_t)n, 1);
        HIPCHK(be::dmalloc((void **)&b->d_cflags, sizeof(int) * cf.size()));
        HIPCHK(be::copy_h2d(b->d_cflags, cf.data(), sizeof(int) * cf.size()));
    }
    for (int i = 0; i < acme_batch::NEV; ++i) {
        HIPCHK(be::event_create(&b->ev0[i]));
        HIPCHK(be::event_create(&b->ev1[i]));
    }
    int rc = init_state(b.get());
    if (rc != ACME_OK) return rc;
    *out = b.release();
    return ACME_OK;
}

extern "C" {

int acme_batch_kernel_variant(const acme_batch *b, int *condensed_rows, int *family) {
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    if (condensed_rows) *condensed_rows = b->generic ? 0 : b->P.shape.nl;
    if (family) *family = !b->generic ? 0 : b->coop_gpw > 0 ? 2 : 1;
    return ACME_OK;
}

int acme_batch_set_progress_callback(acme_batch *b, acme_progress_fn fn, void *user) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    b->progress = fn;
    b->progress_user = user;
    return ACME_OK;
}

int acme_batch_set_host_retention(acme_batch *b, int keep) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    if (!keep && b->retain_host) {
        ON_DEVICE(b);
        HIPCHK(be::device_sync());
        release_reg(b->reg_u);
        release_reg(b->reg_y);
    }
    b->retain_host = keep != 0;
    return ACME_OK;
}

int acme_batch_release_host_buffers(acme_batch *b) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    release_reg(b->reg_u);
    release_reg(b->reg_y);
    return ACME_OK;
}

static void meas_release(acme_batch::Measurement &M) {
    (void)be::dfree(M.d_acc); (void)be::dfree(M.d_tw); (void)be::dfree(M.d_ys);
    (void)be::dfree(M.d_fnum_g); (void)be::dfree(M.d_perm); (void)be::dfree(M.d_sgrp); (void)be::dfree(M.d_wgrp);
    (void)be::dfree(M.d_kbin_g);
    (void)be::dfree(M.d_fold_per); (void)be::dfree(M.d_fold);
    (void)be::dfree(M.d_spec_w); (void)be::dfree(M.d_spec_tw); (void)be::dfree(M.d_spec_acc); (void)be::dfree(M.d_spec_carry);
    (void)be::dfree(M.d_cross_w); (void)be::dfree(M.d_cross_tw); (void)be::dfree(M.d_cross_acc); (void)be::dfree(M.d_cross_carry);
    (void)be::dfree(M.d_tgt); (void)be::dfree(M.d_tgt_which); (void)be::dfree(M.d_tgt_wuni); (void)be::dfree(M.d_tgt_lag); (void)be::dfree(M.d_tgt_acc);
    (void)be::dfree(M.d_wstate); (void)be::dfree(M.d_yw);
    (void)be::dfree(M.d_ens_member); (void)be::dfree(M.d_ens_off); (void)be::dfree(M.d_ens_acc);
    (void)be::dfree(M.d_hist_cnt); (void)be::dfree(M.d_hist_range);
    (void)be::dfree(M.d_ev_lev); (void)be::dfree(M.d_ev_cnt); (void)be::dfree(M.d_ev_idx); (void)be::dfree(M.d_ev_ab);
    (void)be::dfree(M.d_ev_state); (void)be::dfree(M.d_ev_prev);
    M = acme_batch::Measurement{};
}

void acme_batch_destroy(acme_batch *b) {
    if (!b) return;
    join_worker(b);
    DeviceGuard guard_(b->device);
    (void)be::device_sync();
    release_reg(b->reg_u);
    release_reg(b->reg_y);
    (void)be::dfree(b->d_lanec);
    (void)be::dfree(b->d_image); (void)be::dfree(b->d_rowc); (void)be::dfree(b->d_rowi); (void)be::dfree(b->d_state);
    (void)be::dfree(b->d_report); (void)be::dfree(b->d_u); (void)be::dfree(b->d_y); (void)be::dfree(b->d_uv); (void)be::dfree(b->d_uc); (void)be::dfree(b->d_roworder); (void)be::dfree(b->d_cflags); (void)be::dfree(b->d_cache);
    (void)be::dfree(b->d_gh); (void)be::dfree(b->d_ws); (void)be::dfree(b->d_coop_order);
    (void)be::stream_destroy(b->copy_stream);
    (void)be::stream_destroy(b->copy_stream_out);
    (void)be::stream_destroy(b->slow_stream);
    (void)be::dfree(b->d_map_fast); (void)be::dfree(b->d_map_slow);
    (void)be::dfree(b->d_map_bal); (void)be::dfree(b->d_bal_prev); (void)be::dfree(b->d_bal_weight);
    (void)be::flag_free(b->h_u_ready);
    (void)be::dfree(b->os.d_taps); (void)be::dfree(b->os.d_hist_u); (void)be::dfree(b->os.d_hist_y);
    (void)be::dfree(b->os.d_ou); (void)be::dfree(b->os.d_oy); (void)be::dfree(b->os.d_base);
    meas_release(b->meas);
    src_release(b, -1);
    (void)be::dfree(b->src.d_rows); (void)be::dfree(b->src.d_ys);
    for (auto &e : b->os.ev) if (e) (void)be::event_destroy(e);
    for (int i = 0; i < acme_batch::NEV; ++i) {
        if (b->ev0[i]) (void)be::event_destroy(b->ev0[i]);
        if (b->ev1[i]) (void)be::event_destroy(b->ev1[i]);
    }
    delete b;
}

// Two element tables describe the same CIRCUIT STRUCTURE -- the same element kinds in the same residual rows reading the same
// q entries -- when their rows agree in kind, element row and Jq columns (rowi words 0, 1, 3..6); the row constants and the
// flags word (which Gummel-Poon refinements a transistor has: compile-time branches of the reference's closure,
// src/elements.jl:331-396) are what a per-instance table may vary.
static bool same_structure(const std::vector<int> &a, const std::vector<int> &b) {
    if (a.size() != b.size()) return false;
    // (per sub-problem block of 16 rows: the same rows, in whatever order -- a model's rows sit in the lanes by its own
    // pivot-order hint, and an instance's image and tables are packed from the same model)
    auto rows = [](const std::vector<int> &t, size_t blk) {
        std::vector<std::array<int, 6>> r;
        for (int ln = 0; ln < GROUP; ++ln) {
            const size_t at = blk * ROWI * GROUP + ln;
            r.push_back({t[at], t[at + 1 * GROUP], t[at + 3 * GROUP], t[at + 4 * GROUP], t[at + 5 * GROUP], t[at + 6 * GROUP]});
        }
        std::sort(r.begin(), r.end());
        return r;
    };
    for (size_t blk = 0; blk * ROWI * GROUP < a.size(); ++blk)
        if (rows(a, blk) != rows(b, blk)) return false;
    return true;
}
// From now on every instance has its own element tables (each starts as the batch model's).  The 16-lane kernels stage a
// block's 16 tables in LDS next to its images: more LDS per block, possibly the LOW-LDS variant, possibly more than a
// compute unit has.
static int enable_instance_tables(acme_batch *b) {
    if (b->table_stride) return ACME_OK;
    if (!b->generic && b->P.shape.nl > 0)
        return fail(ACME_ERR_UNSUPPORTED, "per-instance element tables on a condensed kernel shape (acme_batch_set_matrices moves such a "
                                          "batch to the plain shape first: rebuild_on_plain_shape)");
    const std::vector<double> &rc = b->generic ? b->G.rowc : b->P.rowc;
    const std::vector<int> &ri = b->generic ? b->G.rowi : b->P.rowi;
    if (!b->generic) {
        const size_t cache_lds = b->o.solver == ACME_SOLVER_CACHING_HOMOTOPY ? (size_t)INST_PER_BLOCK * cache_lds_doubles(b) : 0;
        size_t bytes = sizeof(double) * ((size_t)(b->low ? b->k->lds_low + b->k->lds_tab_low : b->k->lds_per_inst + b->k->lds_tab) + cache_lds);
        if (!b->low && bytes > 160 * 1024 && b->k->low.fn) {
            b->low = true;
            b->kf = &b->k->low;
            bytes = sizeof(double) * ((size_t)b->k->lds_low + b->k->lds_tab_low + cache_lds);
        }
        if (bytes > 160 * 1024) return fail(ACME_ERR_UNSUPPORTED, "per-instance element tables: 16 of them do not fit the LDS of a compute unit for this model");
        b->lds_bytes = bytes;
        HIPCHK(be::set_max_lds(b->kf->fn, (int)b->lds_bytes));
        if (b->kf->fn_jac) HIPCHK(be::set_max_lds(b->kf->fn_jac, (int)b->lds_bytes));
        if (b->kf->fn_solve) HIPCHK(be::set_max_lds(b->kf->fn_solve, (int)b->lds_bytes));
        if (b->kf->fn_stream) HIPCHK(be::set_max_lds(b->kf->fn_stream, (int)b->lds_bytes));
    }
    b->coop_gpw = 0;              // (the cooperative kernel stages ONE table per wave: the lane-per-instance kernel takes over)
    double *drc = nullptr;
    int *dri = nullptr;
    HIPCHK(be::dmalloc((void **)&drc, sizeof(double) * rc.size() * (size_t)b->N));
    HIPCHK(be::dmalloc((void **)&dri, sizeof(int) * ri.size() * (size_t)b->N));
    {
        std::vector<double> all(rc.size() * (size_t)b->N);
        std::vector<int> alli(ri.size() * (size_t)b->N);
        for (long long i = 0; i < b->N; ++i) {
            memcpy(&all[(size_t)i * rc.size()], rc.data(), rc.size() * sizeof(double));
            memcpy(&alli[(size_t)i * ri.size()], ri.data(), ri.size() * sizeof(int));
        }
        HIPCHK(be::copy_h2d(drc, all.data(), all.size() * sizeof(double)));
        HIPCHK(be::copy_h2d(dri, alli.data(), alli.size() * sizeof(int)));
    }
    (void)be::dfree(b->d_rowc);
    (void)be::dfree(b->d_rowi);
    b->d_rowc = drc;
    b->d_rowi = dri;
    b->table_stride = (long long)rc.size();
    b->tablei_stride = (long long)ri.size();
    return ACME_OK;
}

static int state_io(acme_batch *b, double *x, double *p, double *z, const double *cx, const double *cp, const double *cz, bool set);
// A batch on a condensed shape whose instances turn out to differ in their element parameters: the condensed kernels carry no
// per-instance element tables (Shape::TABLES), so the LIBRARY moves the batch to the plain shape -- a new batch built from the
// same model with the condensation switched off takes over every instance: the models earlier calls gave them (inst_models),
// their current state (x and the extrapolation origin, in the caller's layout), the batch's settings.  Solution caches start
// afresh (they are per kernel layout).  acme_batch_kernel_variant reports the shape a batch runs in.
static int rebuild_on_plain_shape(acme_batch *b) {
    acme_batch *nb = nullptr;
    int rc = create_batch(b->host_model, b->N, &b->o, false, &nb);
    if (rc != ACME_OK) return rc;
    struct Destroy { void operator()(acme_batch *p) const { acme_batch_destroy(p); } };
    std::unique_ptr<acme_batch, Destroy> guard(nb);
    if (nb->generic || nb->P.shape.nl > 0) return fail(ACME_ERR_UNSUPPORTED, "no plain kernel shape holds this model's per-instance element parameters");
    // the instances' models, in runs of consecutive instances
    for (long long i = 0; i < b->N && i < (long long)b->inst_models.size();) {
        if (!b->inst_models[(size_t)i]) { ++i; continue; }
        long long j = i;
        std::vector<acme_model> held;
        while (j < (long long)b->inst_models.size() && b->inst_models[(size_t)j] && j - i < 1024) {
            held.push_back(acme_model{*b->inst_models[(size_t)j]});
            ++j;
        }
        std::vector<const acme_model *> ptrs;
        for (const auto &hmod : held) ptrs.push_back(&hmod);
        rc = acme_batch_set_matrices(nb, i, j - i, ptrs.data());
        if (rc != ACME_OK) return rc;
        i = j;
    }
    // where the instances stand (a batch that has run: x, last_p, last_z)
    if (b->samples_done > 0) {
        int npt = 0, nnt = 0;
        for (int k = 0; k < b->P.actual.nsub; ++k) { npt += b->sub_np[k]; nnt += b->sub_nn[k]; }
        std::vector<double> x((size_t)b->N * (b->P.actual.nx ? b->P.actual.nx : 1)), p((size_t)b->N * (npt ? npt : 1)), z((size_t)b->N * (nnt ? nnt : 1));
        rc = state_io(b, x.data(), p.data(), z.data(), nullptr, nullptr, nullptr, false);
        if (rc == ACME_OK) rc = state_io(nb, nullptr, nullptr, nullptr, x.data(), p.data(), z.data(), true);
        if (rc != ACME_OK) return rc;
        nb->samples_done = b->samples_done;
    }
    nb->progress = b->progress;
    nb->progress_user = b->progress_user;
    nb->retain_host = b->retain_host;
    nb->iso_thr = b->iso_thr;
    nb->balance = b->balance;
    std::swap(nb->os, b->os);    // (oversampling: factor, taps, the signals' past and scratch go with the instances)
    std::swap(nb->meas, b->meas);    // (measurements: the window's position and the accumulators, too)
    std::swap(nb->src, b->src);      // (sources: the rows' parameters and the clock)
    std::swap(*b, *nb);          // (b is the plain-shape batch now; the guard destroys what it was)
    return ACME_OK;
}

// the instances acme_batch_set_matrices makes afresh start an oversampled batch's histories from zero (a batch that has not
// run since acme_batch_set_oversampling extends the first samples into the past at its next run instead)
static int os_zero_history(acme_batch *b, long long first, long long count) {
    const acme_batch::Oversampling &O = b->os;
    if (O.k == 1 || O.fresh) return ACME_OK;
    const size_t hu = (size_t)O.du * b->P.actual.nu, hy = (size_t)(O.ld - 1) * b->P.actual.ny;
    std::vector<double> z((size_t)count * (hu > hy ? hu : hy), 0.0);
    if (hu) HIPCHK(be::copy_h2d(O.d_hist_u + (size_t)first * hu, z.data(), sizeof(double) * (size_t)count * hu));
    if (hy) HIPCHK(be::copy_h2d(O.d_hist_y + (size_t)first * hy, z.data(), sizeof(double) * (size_t)count * hy));
    return ACME_OK;
}

int acme_batch_set_matrices(acme_batch *b, long long first, long long count, const acme_model *const *models) {
    join_worker(b);
    if (!b || !models || first < 0 || count < 0 || first + count > b->N) return fail(ACME_ERR_INVALID, "invalid range");
    if (!b->image_stride) return fail(ACME_ERR_INVALID, "batch was not created with per_instance_matrices");
    ON_DEVICE(b);
    // a launch still running on a non-blocking stream writes state / caches / row order back when it
    // ends: let it finish before these are overwritten
    HIPCHK(be::device_sync());
    // Everything is packed and checked BEFORE the batch is touched (ADVICE r5): a model that does not fit leaves it as it was.
    if (b->generic) {
        const size_t img = b->G.image.size();
        const int S = b->G.H.state_total, cd = b->G.H.cache_total;
        std::vector<double> all(img * (size_t)count), st((size_t)count * S), cc((size_t)count * cd);
        std::vector<double> trc;
        std::vector<int> tri;
        bool differ = false, sparse = true;
        for (long long i = 0; i < count; ++i) {
            PackedGeneric G;
            std::string err;
            if (!models[i] || !pack_generic(models[i]->h, G, err, &b->G.H)) return fail(ACME_ERR_UNSUPPORTED, err);
            sparse = sparse && G.H.ell != 0;          // (a model with a fuller matrix row than the batch's sparse forms hold)
            if (!same_structure(G.rowi, b->G.rowi) || G.rowc.size() != b->G.rowc.size() || G.image.size() != img || G.H.ws_total != b->G.H.ws_total)
                return fail(ACME_ERR_INVALID, "per-instance models must share the batch model's dimensions and circuit structure");
            differ = differ || G.rowi != b->G.rowi || G.rowc != b->G.rowc;
            trc.insert(trc.end(), G.rowc.begin(), G.rowc.end());
            tri.insert(tri.end(), G.rowi.begin(), G.rowi.end());
            memcpy(&all[(size_t)i * img], G.image.data(), img * sizeof(double));
            memcpy(&st[(size_t)i * S], G.init_state.data(), S * sizeof(double));
            fresh_cache_generic(G, &cc[(size_t)i * cd]);
        }
        if (differ && !b->table_stride) {
            const int rc_ = enable_instance_tables(b);
            if (rc_ != ACME_OK) return rc_;
        }
        if (!sparse && b->G.H.ell) {          // the whole batch reads the dense matrices from now on (every image has both)
            b->G.H.ell = 0;
            HIPCHK(be::copy_h2d(b->d_gh, &b->G.H, sizeof(GenHeader)));
        }
        if (b->table_stride) {
            HIPCHK(be::copy_h2d(b->d_rowc + (size_t)first * b->table_stride, trc.data(), trc.size() * sizeof(double)));
            HIPCHK(be::copy_h2d(b->d_rowi + (size_t)first * b->tablei_stride, tri.data(), tri.size() * sizeof(int)));
        }
        HIPCHK(be::copy_h2d(b->d_cache + (size_t)first * cd, cc.data(), cc.size() * sizeof(double)));
        HIPCHK(be::copy_h2d(b->d_image + (size_t)first * img, all.data(), all.size() * sizeof(double)));
        if (S) HIPCHK(be::copy_h2d(b->d_state + (size_t)first * S, st.data(), st.size() * sizeof(double)));
        if (b->d_coop_order) {          // (freshly constructed models: no order learnt yet)
            const std::vector<int> ord = coop_initial_order(b->G.H, (size_t)count);
            HIPCHK(be::copy_h2d(b->d_coop_order + (size_t)first * COOP_MAX_N, ord.data(), sizeof(int) * ord.size()));
        }
        return os_zero_history(b, first, count);
    }
    for (int attempt = 0;; ++attempt) {          // (a second pass after a rebuild on the plain shape)
        const size_t img = b->P.image.size();
        const int S = b->k->state;
        const int cd = cache_doubles(b);
        std::vector<double> all(img * (size_t)count), st((size_t)count * S), cc((size_t)count * cd);
        std::vector<double> trc;
        std::vector<int> tri;
        bool differ = false;
        int rare = b->P.rare_kinds;
        for (long long i = 0; i < count; ++i) {
            Packed P;
            std::string err;
            if (!models[i] || !pack_model(models[i]->h, P, err, &b->P.shape, &b->P, b->allow_condense)) return fail(ACME_ERR_UNSUPPORTED, err);
            if (!same_structure(P.rowi, b->P.rowi) || P.rowc.size() != b->P.rowc.size() || P.has_bjt != b->P.has_bjt)
                return fail(ACME_ERR_INVALID, "per-instance models must share the batch model's circuit structure (element kinds, rows, q entries)");
            rare |= P.rare_kinds;       // (an instance whose transistor has Gummel-Poon refinements the batch model's has not)
            differ = differ || P.rowi != b->P.rowi || P.rowc != b->P.rowc;
            trc.insert(trc.end(), P.rowc.begin(), P.rowc.end());
            tri.insert(tri.end(), P.rowi.begin(), P.rowi.end());
            memcpy(&all[(size_t)i * img], P.image.data(), img * sizeof(double));
            // the instance becomes models[i] as freshly constructed: x = 0 and the solvers'
            // extrapolation origin (p = 0, z = that model's init_z), src/ACME.jl:145,253-259
            memcpy(&st[(size_t)i * S], P.init_state.data(), S * sizeof(double));
            fresh_cache(b, P, &cc[(size_t)i * cd]);
        }
        if (differ && !b->table_stride && b->P.shape.nl > 0) {
            // element parameters of their own on a condensed shape: the batch moves to the plain shape by itself
            if (attempt > 0) return fail(ACME_ERR_UNSUPPORTED, "per-instance element parameters: the batch could not be moved off the condensed shape");
            const int rc_ = rebuild_on_plain_shape(b);
            if (rc_ != ACME_OK) return rc_;
            continue;
        }
        if (differ && !b->table_stride) {
            const int rc_ = enable_instance_tables(b);
            if (rc_ != ACME_OK) return rc_;
        }
        b->P.rare_kinds = rare;
        if (b->table_stride) {
            HIPCHK(be::copy_h2d(b->d_rowc + (size_t)first * b->table_stride, trc.data(), trc.size() * sizeof(double)));
            HIPCHK(be::copy_h2d(b->d_rowi + (size_t)first * b->tablei_stride, tri.data(), tri.size() * sizeof(int)));
        }
        HIPCHK(be::copy_h2d(b->d_cache + (size_t)first * cd, cc.data(), cc.size() * sizeof(double)));
        HIPCHK(be::copy_h2d(b->d_image + (size_t)first * img, all.data(), all.size() * sizeof(double)));
        if (S) HIPCHK(be::copy_h2d(b->d_state + (size_t)first * S, st.data(), st.size() * sizeof(double)));
        {
            const int nsub_shape = b->k->d.nsub > 0 ? b->k->d.nsub : 1;
            std::vector<int> ro((size_t)count * nsub_shape * GROUP);
            for (size_t i = 0; i < ro.size(); ++i) ro[i] = (int)(i % GROUP);
            HIPCHK(be::copy_h2d(b->d_roworder + (size_t)first * nsub_shape * GROUP, ro.data(), sizeof(int) * ro.size()));
            std::vector<int> cf((size_t)count, 1);
            HIPCHK(be::copy_h2d(b->d_cflags + (size_t)first, cf.data(), sizeof(int) * cf.size()));
        }
        if (b->P.shape.nl > 0) {          // (a later call may still bring element parameters of its own: keep what a rebuild needs)
            if (b->inst_models.size() != (size_t)b->N) b->inst_models.resize((size_t)b->N);
            for (long long i = 0; i < count; ++i) b->inst_models[(size_t)(first + i)] = std::make_unique<HostModel>(models[i]->h);
        }
        return os_zero_history(b, first, count);
    }
}

// one kernel launch over T samples of device-resident u / y, timed with an event pair
// Re-classify the instances by their iterations per sample since the last classification (only when no launch of the
// slow group is in flight: its members' state is then at rest).  `st`: the stream the fast group runs on.
static int classify_slow(acme_batch *b, be::stream_t st) {
    if (b->samples_done <= b->iso_samples) return ACME_OK;                       // nothing has run since
    if (!b->slow_stream) HIPCHK(be::stream_create_nonblocking(&b->slow_stream));
    if (!b->map_slow.empty() && !be::stream_idle(b->slow_stream)) return ACME_OK;  // keep the groups while the slow one runs
    HIPCHK(be::stream_sync(st));
    HIPCHK(be::stream_sync(b->slow_stream));
    std::vector<long long> w((size_t)b->N * RW_WORDS);
    HIPCHK(be::copy_d2h(w.data(), b->d_report, w.size() * sizeof(long long)));
    if (b->iso_iters.size() != (size_t)b->N) b->iso_iters.assign((size_t)b->N, 0);
    const double dT = (double)(b->samples_done - b->iso_samples);
    std::vector<int> fast, slow;
    for (long long i = 0; i < b->N; ++i) {
        const long long it = w[(size_t)i * RW_WORDS + RW_ITERS_TOTAL];
        const double per = (double)(it - b->iso_iters[(size_t)i]) / dT;
        (per > b->iso_thr ? slow : fast).push_back((int)i);
        b->iso_iters[(size_t)i] = it;
    }
    b->iso_samples = b->samples_done;
    if (slow != b->map_slow || fast != b->map_fast) {
        b->map_fast = fast;
        b->map_slow = slow;
        if (!b->d_map_fast) HIPCHK(be::dmalloc((void **)&b->d_map_fast, sizeof(int) * (size_t)b->N));
        if (!b->d_map_slow) HIPCHK(be::dmalloc((void **)&b->d_map_slow, sizeof(int) * (size_t)b->N));
        if (!fast.empty()) HIPCHK(be::copy_h2d(b->d_map_fast, fast.data(), sizeof(int) * fast.size()));
        if (!slow.empty()) HIPCHK(be::copy_h2d(b->d_map_slow, slow.data(), sizeof(int) * slow.size()));
    }
    return ACME_OK;
}

// Placement of the instances in a launch of the 16-lane kernel (acme_balance.h): how many share a wave, and which wave
// gets which slot.
static int device_cus(acme_batch *b) {
    if (b->cus == 0 && (be::cu_count(&b->cus) != 0 || b->cus <= 0)) b->cus = -1;       // (-1: unknown -- nothing is placed)
    return b->cus;
}
static bool placement_possible(acme_batch *b) {
    return !b->generic && !use_lane_kernel(b) && b->iso_thr == 0.0 && b->map_slow.empty();
}
// instances per wave: 4.  (ACME_WAVE_DENSITY = 2 or 1 in the environment spreads a batch thinner, the waves' other slots
// empty -- measured and NOT adopted: a launch lasts as long as one wave's serial recurrence over the samples, which does
// not get shorter with fewer instances in the wave; BASELINE config 5, 2 048 instances = 512 waves on 1 024 SIMDs:
// 362.9 ms per step at 4 per wave, 362.2 at 2, 444.0 at 1 -- two waves per SIMD then contend.  Kept as a knob: it
// exercises the empty slots an incomplete last wave also has.)
static int wave_density(acme_batch *) {
    if (const char *e = getenv("ACME_WAVE_DENSITY")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) return v; }
    return BAL_SLOTS;
}
// waves placed by their measured cost?  (-1: when the launch has more than one round of blocks)
static bool balance_wanted(acme_batch *b, int per) {
    int mode = b->balance;
    if (const char *e = getenv("ACME_BALANCE")) mode = atoi(e);        // (A/B measurements, tests)
    const long long nu = (b->N + per - 1) / per;
    if (mode >= 0) return mode != 0 && nu >= 2;
    const int cus = device_cus(b);
    return cus > 0 && nu > (long long)WAVES_PER_BLOCK * cus;
}
// The launch's slot -> instance map, on the launch's stream: a first one when the waves are not full (per < 4), a new one
// when enough samples have run since the last (a wave's cost changes slowly along a signal; short real-time launches
// are not each preceded by the two placement kernels).  *slots: what the launch covers (0: no map -- every slot its
// instance).
static int place_waves(acme_batch *b, be::stream_t st, long long *slots) {
    *slots = 0;
    if (!placement_possible(b)) return ACME_OK;
    const int per = wave_density(b);
    const bool bal = balance_wanted(b, per);
    if (per == BAL_SLOTS && !bal) { b->bal_valid = false; return ACME_OK; }
    long long min_samples = 4096;
    if (const char *e = getenv("ACME_BALANCE_MIN_SAMPLES")) min_samples = atoll(e);
    const long long nu = (b->N + per - 1) / per;
    const bool first = !b->bal_valid || b->bal_per != per;
    const bool due = bal && b->samples_done - b->bal_samples >= min_samples;
    if (first && per == BAL_SLOTS && !due) return ACME_OK;        // full waves, nothing measured yet: as they come
    if (first || due) {
        if (!b->d_map_bal) {
            HIPCHK(be::dmalloc((void **)&b->d_map_bal, sizeof(int) * (size_t)b->N * BAL_SLOTS));
            HIPCHK(be::dmalloc((void **)&b->d_bal_weight, sizeof(unsigned) * (size_t)b->N));
            HIPCHK(be::dmalloc((void **)&b->d_bal_prev, sizeof(long long) * (size_t)b->N));
            std::vector<long long> z((size_t)b->N, 0);
            HIPCHK(be::copy_h2d(b->d_bal_prev, z.data(), sizeof(long long) * z.size()));
        }
        BalArgs B{};
        B.report = b->d_report;
        B.prev = b->d_bal_prev;
        B.weight = b->d_bal_weight;
        B.map = b->d_map_bal;
        B.n = b->N;
        B.per = per;
        B.nu = (int)nu;
        B.first_round = device_cus(b) > 0 ? WAVES_PER_BLOCK * b->cus : 0;
        HIPCHK(be::launch_balance(B, st));
        b->bal_samples = b->samples_done;
        b->bal_valid = true;
        b->bal_per = per;
    }
    *slots = nu * BAL_SLOTS;
    return ACME_OK;
}

static void fill_gargs(const acme_batch *b, GArgs &A) {
    A.H = b->d_gh;
    A.image = b->d_image;
    A.image_stride = b->image_stride;
    A.rowc = b->d_rowc;
    A.rowi = b->d_rowi;
    A.table_stride = b->table_stride;
    A.tablei_stride = b->tablei_stride;
    A.state = b->d_state;
    A.report = b->d_report;
    A.cache = b->d_cache;
    A.ws = b->d_ws;
    A.n_inst = b->N;
    A.sample_base = b->samples_done;
    A.tol = b->o.tol;
    A.maxiter = b->o.maxiter;
    A.solver = b->o.solver;
    A.mode = GEN_RUN;
}

// The event ring around the launches: ev_take retires the oldest pair when the ring is full and records the start event
// of the next slot on `st`; ev_commit records its end event behind the launches and counts the launch's T samples.
static int ev_take(acme_batch *b, be::stream_t st, int *slot) {
    if (b->ev_pending == acme_batch::NEV) {
        int rc_ = drain_events(b, 1);
        if (rc_ != ACME_OK) return rc_;
    }
    *slot = (b->ev_head + b->ev_pending) % acme_batch::NEV;
    HIPCHK(be::event_record(b->ev0[*slot], st));
    return ACME_OK;
}
static int ev_commit(acme_batch *b, be::stream_t st, int slot, long long T, int *slot_out) {
    HIPCHK(be::event_record(b->ev1[slot], st));
    ++b->ev_pending;
    b->samples_done += T;
    if (slot_out) *slot_out = slot;
    return ACME_OK;
}

static int launch_run(acme_batch *b, const double *du, double *dy, long long T, be::stream_t st, int *slot_out,
                      long long u_stride = 0, long long y_stride = 0, const long long *u_ready = nullptr) {
    int slot = 0, rc_;
    if (b->generic) {
        GArgs A{};
        fill_gargs(b, A);
        A.u = du;
        A.y = dy;
        A.T = T;
        if ((rc_ = ev_take(b, st, &slot)) != ACME_OK) return rc_;
        if (b->coop_gpw > 0) {
            fill_coop(b, A);
            HIPCHK(be::launch_coop(A, coop_lds_bytes(b->G.H, b->coop_imgl != 0, b->coop_wpb, b->coop_gpw, b->coop_nc), st));
        } else {
            HIPCHK(be::launch_generic(A, st));
        }
        return ev_commit(b, st, slot, T, slot_out);
    }
    KArgs A{};
    fill_args(b, A);
    A.u = du;
    A.y = dy;
    A.T = T;
    A.u_stride = u_stride;
    A.y_stride = y_stride;
    A.u_ready = u_ready;
    const unsigned grid = (unsigned)((b->N + INST_PER_BLOCK - 1) / INST_PER_BLOCK);
    if (b->iso_thr > 0.0 && !use_lane_kernel(b)) {
        rc_ = classify_slow(b, st);
        if (rc_ != ACME_OK) return rc_;
    }
    if (!b->map_slow.empty() && !use_lane_kernel(b)) {
        // two launches: the slow instances on their own stream, everything else on the caller's (timed by the events)
        KArgs F = A, S_ = A;
        F.inst_map = b->d_map_fast; F.n_inst = (long long)b->map_fast.size();
        S_.inst_map = b->d_map_slow; S_.n_inst = (long long)b->map_slow.size();
        // (the slow group's launch is ordered behind everything the caller has queued on `st` -- the copy that brings
        // its u in, a kernel that still reads the buffer y goes to: its stream waits for this point of the caller's)
        if ((rc_ = ev_take(b, st, &slot)) != ACME_OK) return rc_;
        HIPCHK(be::stream_wait_event(b->slow_stream, b->ev0[slot]));
        HIPCHK(b->kf->launch(S_, (unsigned)((S_.n_inst + INST_PER_BLOCK - 1) / INST_PER_BLOCK), b->lds_bytes, b->slow_stream));
        if (F.n_inst > 0) HIPCHK(b->kf->launch(F, (unsigned)((F.n_inst + INST_PER_BLOCK - 1) / INST_PER_BLOCK), b->lds_bytes, st));
        return ev_commit(b, st, slot, T, slot_out);
    }
    if ((rc_ = ev_take(b, st, &slot)) != ACME_OK) return rc_;
    if (use_lane_kernel(b)) {
        // instances per wave: as few as still give every SIMD of the chip (1 024) no more than one wave -- the
        // batch's run time is one wave's, and a wave's Newton loop lasts as long as its slowest lane's
        // (ACME_LANE_DENSITY in the environment overrides: A/B measurements)
        int dens = 64;
        while (dens > 4 && (b->N + dens / 2 - 1) / (dens / 2) <= 1024) dens /= 2;
        if (const char *e = getenv("ACME_LANE_DENSITY")) { const int v = atoi(e); if (v >= 1 && v <= 64) dens = v; }
        A.lane_density = dens;
        const long long per_block = (long long)WAVES_PER_BLOCK * dens;
        HIPCHK(b->k->launch_lane(A, (unsigned)((b->N + per_block - 1) / per_block), lane_lds_bytes(b), st));
    }
    else {
        long long slots = 0;
        rc_ = place_waves(b, st, &slots);
        if (rc_ != ACME_OK) return rc_;
        // (a streamed host-buffer run: the kernel variant that waits for its u tiles to land, KArgs::u_ready)
        const auto launch = u_ready ? b->kf->launch_stream : b->kf->launch;
        if (!launch) return fail(ACME_ERR_INVALID, "this model's kernel has no streamed variant");
        if (slots > 0) {
            A.inst_map = b->d_map_bal;
            A.n_inst = slots;
            HIPCHK(launch(A, (unsigned)((slots + INST_PER_BLOCK - 1) / INST_PER_BLOCK), b->lds_bytes, st));
        } else
            HIPCHK(launch(A, grid, b->lds_bytes, st));
    }
    return ev_commit(b, st, slot, T, slot_out);
}

// soft: a staging buffer that cannot be had is no error (the caller takes another path) and leaves none behind
static int ensure_staging(acme_batch *b, size_t nub, size_t nyb, bool soft = false) {
    if (nub > b->cap_u) {
        (void)be::dfree(b->d_u); b->d_u = nullptr; b->cap_u = 0;
        if (soft) { if (be::dmalloc_try((void **)&b->d_u, nub) != 0) { b->d_u = nullptr; return ACME_ERR_HIP; } }
        else HIPCHK(be::dmalloc((void **)&b->d_u, nub));
        b->cap_u = nub;
    }
    if (nyb > b->cap_y) {
        (void)be::dfree(b->d_y); b->d_y = nullptr; b->cap_y = 0;
        HIPCHK(be::dmalloc((void **)&b->d_y, nyb));
        b->cap_y = nyb;
    }
    return ACME_OK;
}

// A streamed host run launches the kernel FIRST and lets its waves wait for u to land (KArgs::u_ready): every block of
// the grid must be resident from the start -- a block that waits for a compute unit behind blocks that wait for data
// would be fine, but the data's copy must never depend on a kernel that cannot finish, so the streamed path is only
// taken when the whole grid fits the chip in one round (two blocks per compute unit up to 80 KB of LDS each, else one).
static bool streamed_fits(const acme_batch *b) {
    int cus = 0;
    if (be::cu_count(&cus) != 0 || cus <= 0) return true;       // (the emulator: launches are synchronous there)
    const long long per_cu = b->lds_bytes <= 80u * 1024u ? 2 : 1;
    const long long blocks = (b->N + INST_PER_BLOCK - 1) / INST_PER_BLOCK;
    return blocks <= per_cu * cus;
}

}  // extern "C" (the pipeline's driver is a template)

// ---- host-buffer runs in time slices ------------------------------------------------------------------------------------------
// Long runs on host arrays go through HBM in time slices, two staging buffers each way: while slice s computes (state
// carries over from launch to launch, bit-identically), copy_stream brings in the input rows of slice s + 1 and
// copy_stream_out takes out the output rows of slice s - 1.  Slices is such a run's geometry, run_slices its ordering.
struct Slices {
    long long T, TS;                // samples of the run, of a slice (the last one may be shorter)
    size_t N;
    int nin, nout;                  // rows per sample that come in / go out
    const double *u;                // the caller's [N][T][nin] ...
    double *y;                      // ... and [N][T][nout]; NULL: the outputs are not kept
    double *d_in, *d_out;           // staging, two slices each: slice s uses half s & 1
    be::stream_t cs, cso;
    long long ns() const { return (T + TS - 1) / TS; }
    long long len(long long s) const { return (s + 1) * TS <= T ? TS : T - s * TS; }
    double *in(long long s) const { return d_in + (s & 1) * (N * (size_t)TS * nin); }
    double *out(long long s) const { return y ? d_out + (s & 1) * (N * (size_t)TS * nout) : nullptr; }
    int copy_in(long long s) const {            // (packed: an instance's rows len(s) apart)
        if (!nin) return 0;
        const size_t w = sizeof(double) * (size_t)len(s) * nin;
        return be::copy2d_h2d_async(in(s), w, u + (size_t)s * TS * nin, sizeof(double) * (size_t)T * nin, w, N, cs);
    }
    int copy_out(long long s) const {
        if (!nout || !y) return 0;
        const size_t w = sizeof(double) * (size_t)len(s) * nout;
        return be::copy2d_d2h_async(y + (size_t)s * TS * nout, sizeof(double) * (size_t)T * nout, out(s), w, w, N, cso);
    }
};
static int copy_streams(acme_batch *b, bool out) {
    if (!b->copy_stream) HIPCHK(be::stream_create_nonblocking(&b->copy_stream));
    if (out && !b->copy_stream_out) HIPCHK(be::stream_create_nonblocking(&b->copy_stream_out));
    return ACME_OK;
}
// The slice length of the fully staged pipeline: only the first copy-in and the last copy-out are exposed, so many small
// slices -- 24 for a second of audio: a launch costs microseconds, a slice of the headline workload 0.5 GB of copies
static long long staged_slice(long long T) {
    if (T < 4096) return T;
    long long want = 24;
    if (const char *es = getenv("ACME_HOST_STAGED_SLICES")) { const long long v = atoll(es); if (v >= 1 && v <= 4096) want = v; }
    const long long TS = ((T / want + CHUNK - 1) / CHUNK) * CHUNK;
    if (TS < 1024 && want <= 24) return 1024;
    return TS < CHUNK ? CHUNK : TS;
}
// How a slice's outputs leave, the default: the calling thread issues the copy on copy_stream_out -- behind the copy-in of
// the same step: from pageable memory the call of a copy-out returns when the copy is done, that of a copy-in earlier
struct CopyOut {
    const Slices &g;
    int ready(long long) { return 0; }          // (wait() has seen every earlier copy out)
    int hand_over(long long) { return 0; }
    int issue(long long s) { return g.copy_out(s); }
    int wait() { return be::stream_sync(g.cso); }
    int last(long long s) { const int rc = g.copy_out(s); return rc != 0 ? rc : be::stream_sync(g.cso); }
};
// ... and through a helper thread per slice, for copies that block the thread that issues them
struct ThreadCopyOut {
    const Slices &g;
    const int dev;
    std::future<int> done[2] = {};
    int blocking(long long s) const {
        DeviceGuard d(dev);
        if (d.rc != 0) return d.rc;
        const int rc = g.copy_out(s);
        return rc != 0 ? rc : be::stream_sync(g.cso);
    }
    int ready(long long s) { return done[s & 1].valid() ? done[s & 1].get() : 0; }     // the y rows of slice s-2 have left
    int hand_over(long long s) { done[s & 1] = std::async(std::launch::async, [this, s] { return blocking(s); }); return 0; }
    int issue(long long) { return 0; }
    int wait() { return 0; }                    // (the slices overlap; ready() waits when the buffer is needed)
    int last(long long s) {
        for (long long k = 0; k < 2; ++k) if (const int rc = ready(k)) return rc;
        return blocking(s);
    }
    ~ThreadCopyOut() { for (auto &f : done) if (f.valid()) (void)f.get(); }             // (an error return: no thread is left behind)
};
// The pipeline.  enqueue(s, in, out, n, &done) puts slice s -- n samples, inputs in `in`, outputs to `out` -- on the launch
// stream and names the event that marks it done; `out` is how the outputs leave (CopyOut, ThreadCopyOut).  Slice s is
// enqueued before slice s-1 is waited for, so the device never idles between them; the copies of s+1 and s-1 run beside it.
template <class Enqueue, class Out>
static int run_slices(acme_batch *b, const Slices &g, Enqueue enqueue, Out &&out) {
    const long long ns = g.ns();
    be::event_t prev{}, done{};
    HIPCHK(g.copy_in(0));
    HIPCHK(be::stream_sync(g.cs));
    for (long long s = 0; s < ns; ++s, prev = done) {
        HIPCHK(out.ready(s));                                           // out(s) may be written
        const int rc = enqueue(s, g.in(s), g.out(s), g.len(s), &done);
        if (rc != ACME_OK) return rc;
        if (s > 0) HIPCHK(be::event_sync(prev));                        // slice s-1 done: its buffers are free
        if (s > 0 && b->slow_stream) HIPCHK(be::stream_sync(b->slow_stream));   // (... the isolated slow group's, too)
        // (hand_over and issue are two hooks on purpose: a hand-over to a helper thread must come BEFORE the copy-in, whose
        // call may block, a copy-out on the stream stays BEHIND it -- merging them changes one caller's order)
        if (s > 0) HIPCHK(out.hand_over(s - 1));
        if (s + 1 < ns) HIPCHK(g.copy_in(s + 1));                       // both overlap slice s, and each other
        if (s > 0) HIPCHK(out.issue(s - 1));
        if (s + 1 < ns) HIPCHK(be::stream_sync(g.cs));
        if (s > 0) HIPCHK(out.wait());
        if (s > 0 && b->progress) b->progress(b->progress_user, s * g.TS, g.T);
    }
    HIPCHK(be::event_sync(prev));
    if (b->slow_stream) HIPCHK(be::stream_sync(b->slow_stream));
    HIPCHK(out.last(ns - 1));
    if (b->progress) b->progress(b->progress_user, g.T, g.T);
    return ACME_OK;
}

extern "C" {

// ---- oversampled runs (acme_batch_set_oversampling) and measured runs (acme_batch_set_measurement) ----------------------
// Time slice by time slice on the launch stream: [put the full input rows together (run_const)] -> interpolate to the model
// rate (acme_resample.h) -> the UNCHANGED run kernel over k x the slice's samples -> decimate -> [measure the slice's
// base-rate outputs (acme_measure.h)]; the histories carry the signals' past from slice to slice and call to call.  The
// model-rate scratch is one slice's (ACME_OS_SLICE base-rate samples, default 4 096: config 5 -- 2 048 instances at k = 4 --
// 0.8 GB).  Host buffers: run_slices, as run_impl's staged pipeline; never the streamed path.
// k = 1 (a measurement without oversampling): there is nothing to resample -- the run kernel reads the slice's input rows and
// writes its outputs where the measurement reads them.  Device arrays with y stored run as ONE slice, the launch a plain run
// makes; y = NULL: outputs go to one slice of scratch (meas.d_ys) and are never copied anywhere.
static long long os_slice(long long T) {
    long long TS = 4096;
    if (const char *e = getenv("ACME_OS_SLICE")) { const long long v = atoll(e); if (v >= 1) TS = v; }
    return T < TS ? T : TS;
}
// the source kernel keeps TABLE rows in LDS unless ACME_SOURCE_LDS=0 (A/B measurements, tests)
static bool source_lds() {
    const char *e = getenv("ACME_SOURCE_LDS");
    return !(e && e[0] == '0');
}
static int os_grow(double **p, size_t *cap, size_t bytes) {
    if (bytes > *cap) {
        (void)be::dfree(*p); *p = nullptr; *cap = 0;
        HIPCHK(be::dmalloc((void **)p, bytes));
        *cap = bytes;
    }
    return ACME_OK;
}
// the measurement step of n base-rate output samples (instance i, sample t, row r at y[(i * pitch + t) * ny + r]) that follow
// the meas.pos samples since arming: the part inside the window [start, start + length), chunk by chunk.  u: the same n samples
// of the base-rate input rows, complete (instance i, sample t, row r at u[(i * upitch + t) * nu + r]); the cross-spectrum reads it.
// packed: y holds the measured rows alone, [N][pitch][nrows] (the weighted rows of meas_feed) -- ny = nrows, the identity row table
static int meas_step(acme_batch *b, const double *y, long long n, long long pitch, const double *u, long long upitch, be::stream_t st,
                     bool packed = false) {
    acme_batch::Measurement &M = b->meas;
    unsigned char row[64];
    for (int r = 0; r < 64; ++r) row[r] = packed ? (unsigned char)r : M.row[r];
    const long long end = M.W ? M.start + (M.W - 1) * M.hop + M.win : M.length ? M.start + M.length : LLONG_MAX;
    const long long lo = M.pos > M.start ? M.pos : M.start, hi = M.pos + n < end ? M.pos + n : end;
    for (long long s = lo; M.nrows > 0 && s < hi; s += M.chunk) {
        const long long len = hi - s < M.chunk ? hi - s : M.chunk;
        MeasArgs A{y, M.d_acc, M.d_tw, b->N, len, pitch, s - M.pos, packed ? M.nrows : b->P.actual.ny, M.nrows, M.H, {}};
        memcpy(A.row, row, sizeof(A.row));
        if (M.W) {      // a series: the chunk's table and ONE kernel, whatever windows the chunk holds
            const MeasSeries S{M.win, M.hop, M.W, s - M.start};
            const MeasSeriesTwArgs W{M.d_tw, M.bins ? M.d_kbin_g : M.pi ? M.d_fnum_g : nullptr, M.f_num, M.f_den, len, S, M.H,
                                     M.pi ? M.F : 1, M.bins ? 1 : 0};
            HIPCHK(meas_series_launch(W, MeasSeriesArgs{MeasPiArgs{A, M.d_perm, M.d_sgrp, M.d_wgrp}, S}, M.pi, st));
            continue;
        }
        if (M.bins) {
            const MeasBinsTwArgs W{M.d_tw, M.d_kbin_g, s - M.start, len, M.f_den, M.H, M.F};
            HIPCHK(meas_bins_launch(W, MeasPiArgs{A, M.d_perm, M.d_sgrp, M.d_wgrp}, st));
        } else if (M.pi) {
            const MeasPiTwArgs W{M.d_tw, M.d_fnum_g, s - M.start, len, M.f_den, M.H, M.F};
            HIPCHK(meas_pi_launch(W, MeasPiArgs{A, M.d_perm, M.d_sgrp, M.d_wgrp}, st));
        } else {
            const MeasTwArgs W{M.d_tw, s - M.start, len, M.f_num, M.f_den, M.H};
            HIPCHK(meas_launch(W, A, st));
        }
        if (M.fold) {   // one more kernel on the same chunk of y
            MeasFoldArgs G{y, M.d_fold, M.d_fold_per, b->N, len, pitch, s - M.pos, s - M.start, M.fold_pmax, A.ny, M.nrows, {}};
            memcpy(G.row, row, sizeof(G.row));
            HIPCHK(meas_fold_launch(G, st));
        }
        if (M.spec) {   // ... and the segments that end in this chunk
            MeasSpecArgs G{y, M.d_spec_acc, M.d_spec_carry, M.d_spec_w, M.d_spec_tw, b->N, len, pitch, s - M.pos, s - M.start,
                           M.spec_L, M.spec_hop, A.ny, M.nrows, {}};
            memcpy(G.row, row, sizeof(G.row));
            HIPCHK(meas_spectrum_launch(G, st));
        }
        if (M.cross) {  // ... and those segments of the input row beside the measured rows
            MeasCrossArgs G{{y, M.d_cross_acc, M.d_cross_carry, M.d_cross_w, M.d_cross_tw, b->N, len, pitch, s - M.pos, s - M.start,
                             M.cross_L, M.cross_hop, A.ny, M.nrows, {}}, u, upitch, b->P.actual.nu, M.cross_in};
            memcpy(G.S.row, row, sizeof(G.S.row));
            HIPCHK(meas_cross_launch(G, st));
        }
        if (M.target) { // ... and the residual against the target on the same chunk
            MeasTargetArgs G{y, M.d_tgt_acc, M.d_tgt, M.d_tgt_which, M.d_tgt_lag, M.d_tgt_wuni, b->N, len, pitch, s - M.pos, s - M.start,
                             M.tgt_P, M.tgt_c, A.ny, M.nrows, {}};
            memcpy(G.row, row, sizeof(G.row));
            HIPCHK(meas_target_launch(G, st));
        }
        if (M.ens) {    // ... and the statistics across the groups' instances at the chunk's recorded samples
            const size_t plane = (size_t)M.ens_G * M.nrows * (size_t)M.ens_E;
            MeasEnsArgs G{y, M.d_ens_acc, (long long *)(M.d_ens_acc + 4 * plane), M.d_ens_member, M.d_ens_off, len, pitch, s - M.pos,
                          s - M.start, M.ens_stride, M.ens_E, 0, 0, M.ens_G, A.ny, M.nrows, {}};
            meas_ensemble_range(G.m0, len, G.stride, &G.e0, &G.nrec);
            memcpy(G.row, row, sizeof(G.row));
            HIPCHK(meas_ensemble_launch(G, st));
        }
        if (M.hist) {   // ... and every sample of the chunk into one counter of its pair
            MeasHistArgs G{y, M.d_hist_cnt, M.d_hist_range, b->N, len, pitch, s - M.pos, M.hist_B, M.hist_mode, A.ny, M.nrows, {}};
            memcpy(G.row, row, sizeof(G.row));
            HIPCHK(meas_hist_launch(G, st));
        }
        if (M.events) { // ... and through the levels' automata, from where the chunk before left them
            MeasEventsArgs G{y, M.d_ev_lev, M.d_ev_cnt, M.d_ev_idx, M.d_ev_ab, M.d_ev_state, M.d_ev_prev, b->N, len, pitch, s - M.pos,
                             s - M.start, M.ev_C, M.ev_E, A.ny, M.nrows, {}};
            memcpy(G.row, row, sizeof(G.row));
            HIPCHK(meas_events_launch(G, st));
        }
    }
    M.pos += n;
    return ACME_OK;
}
// what a slice hands to the measurement: meas_step on its outputs, or -- a weighting is set -- on the weighted measured rows.
// The cascade runs over every sample since arming (its states carry from slice to slice), one kernel per stretch of at most
// os_slice samples into meas.d_yw, and meas_step reads that packed array; the cross-spectrum's u is the slice's own.  Once the
// window has ended nothing reads the weighted signal any more and the filter stops with it.
static int meas_feed(acme_batch *b, const double *y, long long n, long long pitch, const double *u, long long upitch, be::stream_t st) {
    acme_batch::Measurement &M = b->meas;
    if (!M.wS || M.nrows == 0) return meas_step(b, y, n, pitch, u, upitch, st);
    const long long end = M.W ? M.start + (M.W - 1) * M.hop + M.win : M.length ? M.start + M.length : LLONG_MAX;
    if (M.pos >= end) { M.pos += n; return ACME_OK; }
    const int ny = b->P.actual.ny, nu = b->P.actual.nu;
    const long long WS = os_slice(n);
    const int rc = os_grow(&M.d_yw, &M.cap_yw, sizeof(double) * (size_t)b->N * (size_t)WS * (size_t)M.nrows);
    if (rc != ACME_OK) return rc;
    for (long long off = 0; off < n; off += WS) {
        const long long len = n - off < WS ? n - off : WS;
        MeasWeightArgs G{y + off * ny, M.d_yw, M.d_wstate, b->N, len, pitch, ny, M.nrows, M.wS, {}, {}};
        memcpy(G.sos, M.wsos, sizeof(G.sos));
        memcpy(G.row, M.row, sizeof(G.row));
        HIPCHK(meas_weight_launch(G, st));
        const int rs = meas_step(b, M.d_yw, len, len, u ? u + off * nu : nullptr, upitch, st, true);
        if (rs != ACME_OK) return rs;
    }
    return ACME_OK;
}
// u: [N][T][nu], or -- const_mask != 0 -- the varying rows [N][T][nuv] and u_const [N][nu] (acme_batch_run_const); y: [N][T][ny],
// or NULL (a measured run that stores no outputs).  sourced (acme_batch_run_sources): u holds the rows without a source
// [N][T][nin] (NULL when there is none), the source kernel (acme_source.h) puts the slice's full rows together where the
// expand kernel does for constant rows, the CONST rows are held, and the source clock advances slice by slice; always
// sliced -- the batch owns one slice of input rows, never [N][T][nu]
static int run_os(acme_batch *b, const double *u, const double *u_const, unsigned long long const_mask, double *y, long long T,
                  int mem, be::stream_t st, bool sourced = false) {
    acme_batch::Oversampling &O = b->os;
    acme_batch::Measurement &M = b->meas;
    const int k = O.k, nu = b->P.actual.nu, ny = b->P.actual.ny;
    const size_t N = (size_t)b->N;
    int nin = nu;                               // rows of u as the caller hands them over
    if (sourced) const_mask = b->src.cmask;
    for (int r = 0; r < nu && r < 64; ++r) nin -= ((sourced ? b->src.mask : const_mask) >> r & 1ull) ? 1 : 0;
    const bool host = mem == ACME_MEM_HOST, expand = !sourced && const_mask != 0ull, keep = y != nullptr;
    const long long TS = k == 1 && !host && keep && !sourced ? T : os_slice(T), ns = (T + TS - 1) / TS;
    // (k = 1: the slices of caller's device arrays are packed into d_base when they are not whole)
    const bool pack = k == 1 && !host && !expand && !sourced && nu && ns > 1;
    // (sourced, k = 1, y in device memory: the run kernel writes a slice's outputs packed; they go to y from scratch)
    const bool scatter = sourced && k == 1 && !host && keep && ny && ns > 1;
    const bool use_lds = source_lds();
    int rc = ACME_OK;
    if (k > 1) rc = os_grow(&O.d_ou, &O.cap_ou, sizeof(double) * N * (size_t)(k * TS) * nu);
    if (rc == ACME_OK && k > 1) rc = os_grow(&O.d_oy, &O.cap_oy, sizeof(double) * N * (size_t)(k * TS) * ny);
    if (rc == ACME_OK && (expand || pack || sourced)) rc = os_grow(&O.d_base, &O.cap_base, sizeof(double) * N * (size_t)TS * nu);
    if (rc == ACME_OK && scatter) rc = os_grow(&b->src.d_ys, &b->src.cap_ys, sizeof(double) * N * (size_t)TS * ny);
    if (rc == ACME_OK && !keep) rc = os_grow(&M.d_ys, &M.cap_ys, sizeof(double) * N * (size_t)TS * ny);
    if (rc == ACME_OK && host) rc = ensure_staging(b, 2 * sizeof(double) * N * (size_t)TS * nin, keep ? 2 * sizeof(double) * N * (size_t)TS * ny : 0);
    if (rc == ACME_OK && host && expand) rc = os_grow(&b->d_uc, &b->cap_uc, sizeof(double) * N * (size_t)nu);
    if (rc != ACME_OK) return rc;
    const double *uc = u_const;
    if (host && expand) {
        HIPCHK(be::copy_h2d_async(b->d_uc, u_const, sizeof(double) * N * (size_t)nu, st));
        uc = b->d_uc;
    }
    const double *g = O.d_taps, *h = O.d_taps + O.lu;
    // slice s of n samples on the launch stream: inputs at src, an instance's rows `pitch` samples apart; host arrays: base-rate
    // outputs to ydst
    auto slice = [&](long long s, const double *src, long long pitch, double *ydst, long long n) -> int {
        const long long nk = n * k;
        if (expand || pack) {
            HIPCHK(be::launch_expand(O.d_base, src, expand ? uc : src, const_mask, (long long)N, n, pitch, nu, nin, st));
            src = O.d_base;
            pitch = n;
        }
        if (sourced && nu) {
            SrcArgs A{O.d_base, nin ? src : nullptr, b->src.d_rows, (long long)N, n, n, pitch, b->src.clock, nu, nin, 0, 0ull};
            src_plan(A, b->src.row, use_lds);
            HIPCHK(src_launch(A, st));
            src = O.d_base;
            pitch = n;
        }
        if (sourced) b->src.clock += n;
        // the slice's base-rate outputs
        double *dst = !keep ? M.d_ys : host ? ydst : scatter ? b->src.d_ys : y + (size_t)s * TS * ny;
        const long long ypitch = keep && !host && !scatter ? T : n;
        if (k == 1) {
            const int rc_ = launch_run(b, src, dst, n, st, nullptr);
            if (rc_ != ACME_OK) return rc_;
        } else {
            if (nu) {
                OsHistArgs H{O.d_hist_u, src, (long long)N, n, pitch, nu, O.du};
                if (O.fresh) HIPCHK(os_launch_hist(H, true, st));
                const OsInterpArgs I{src, O.d_hist_u, O.d_ou, g, (long long)N, n, pitch, nu, O.lu, O.du, O.held | const_mask};
                HIPCHK(os_launch_interp(k, I, st));
                HIPCHK(os_launch_hist(H, false, st));
            }
            const int rc_ = launch_run(b, O.d_ou, O.d_oy, nk, st, nullptr);
            if (rc_ != ACME_OK) return rc_;
            if (ny) {
                OsHistArgs H{O.d_hist_y, O.d_oy, (long long)N, nk, nk, ny, O.ld - 1};
                if (O.fresh) HIPCHK(os_launch_hist(H, true, st));
                const OsDecimArgs D{O.d_oy, O.d_hist_y, dst, h, (long long)N, n, ypitch, k, ny, O.ld};
                HIPCHK(os_launch_decim(D, st));
                HIPCHK(os_launch_hist(H, false, st));
            }
            O.fresh = false;
        }
        if (scatter) HIPCHK(src_launch_copy(SrcCopyArgs{y + (size_t)s * TS * ny, dst, (long long)N, n, T, ny}, st));
        return M.on ? meas_feed(b, dst, n, ypitch, src, pitch, st) : ACME_OK;
    };
    if (!host) {
        for (long long s = 0; s < ns; ++s) {
            rc = slice(s, u + (size_t)s * TS * nin, T, nullptr, (s + 1) * TS <= T ? TS : T - s * TS);
            if (rc != ACME_OK) return rc;
        }
        if (b->progress) b->progress(b->progress_user, T, T);
        return ACME_OK;
    }
    if (!b->retain_host) { release_reg(b->reg_u); release_reg(b->reg_y); }
    else {
        (void)ensure_registered(b->reg_u, u, sizeof(double) * N * (size_t)T * (nin ? nin : 1));
        if (keep) (void)ensure_registered(b->reg_y, y, sizeof(double) * N * (size_t)T * ny);
    }
    if ((rc = copy_streams(b, true)) != ACME_OK) return rc;
    const Slices sl{T, TS, N, nin, ny, u, y, b->d_u, b->d_y, b->copy_stream, b->copy_stream_out};
    return run_slices(b, sl, [&](long long s, const double *in, double *out, long long n, be::event_t *done) -> int {
        const int rc_ = slice(s, in, n, out, n);
        if (rc_ != ACME_OK) return rc_;
        HIPCHK(be::event_record(*done = O.ev[s & 1], st));       // (slice s has been decimated and measured)
        return ACME_OK;
    }, CopyOut{sl});      // (progress in base-rate samples)
}

static int run_impl(acme_batch *b, const double *u, double *y, long long T, int mem, void *stream);
int acme_batch_run(acme_batch *b, const double *u, double *y, long long T, int mem, void *stream) {
    RunGuard serial(b);
    if (b && b->src.armed) return fail(ACME_ERR_INVALID, "acme_batch_run: input rows have sources (acme_batch_set_source_*); use acme_batch_run_sources");
    return run_impl(b, u, y, T, mem, stream);
}
static int run_impl(acme_batch *b, const double *u, double *y, long long T, int mem, void *stream) {
    if (!b || T < 0) return fail(ACME_ERR_INVALID, "invalid argument to acme_batch_run");
    const int nu = b->P.actual.nu, ny = b->P.actual.ny;
    // (y = NULL: a measured run that stores no outputs -- only while a measurement is armed)
    if ((nu > 0 && T > 0 && !u) || (ny > 0 && T > 0 && !y && !b->meas.on)) return fail(ACME_ERR_INVALID, "null u or y");
    if (T == 0) return ACME_OK;
    ON_DEVICE(b);
    be::stream_t st = (be::stream_t)stream;
    if (b->os.k > 1 || b->meas.on) {
        if (mem != ACME_MEM_HOST && mem != ACME_MEM_DEVICE) return fail(ACME_ERR_INVALID, "mem must be ACME_MEM_HOST or ACME_MEM_DEVICE");
        return run_os(b, u, nullptr, 0ull, y, T, mem, st);
    }
    if (mem == ACME_MEM_DEVICE) {
        const int rc_ = launch_run(b, u, y, T, st, nullptr);
        if (rc_ == ACME_OK && b->progress) b->progress(b->progress_user, T, T);
        return rc_;
    }
    if (mem != ACME_MEM_HOST) return fail(ACME_ERR_INVALID, "mem must be ACME_MEM_HOST or ACME_MEM_DEVICE");

    // Host buffers.  Long runs go through HBM in time slices (Slices / run_slices above).
    const size_t N = (size_t)b->N;
    // Page-locking (and with it every path that lets the device touch the caller's arrays directly) is for callers who
    // have promised to keep the arrays alive while they stay locked: acme_batch_set_host_retention.  Everyone else gets
    // the staged pipeline from ordinary memory below -- which is also the faster ONE-SHOT call: locking 14.4 GB costs
    // 0.4 s, more than the whole run (headline: 0.39 s staged from pageable memory, 0.70 s locked + streamed, 0.30 s
    // streamed from arrays that are locked already).
    if (!b->retain_host) { release_reg(b->reg_u); release_reg(b->reg_y); }
    const bool lock_u = !nu || (b->retain_host && ensure_registered(b->reg_u, u, sizeof(double) * N * (size_t)T * nu));
    const bool lock_y = !ny || (b->retain_host && ensure_registered(b->reg_y, y, sizeof(double) * N * (size_t)T * ny));
    // Direct access: page-locked host memory is mapped into the device's address space, so the kernel can read its u tiles
    // from, and write its y tiles to, the caller's arrays over the bus itself (KArgs::u_stride / y_stride: a time slice
    // of the arrays in place).  Writes are posted and y is the smaller stream: y ALWAYS goes that way -- no staging, no
    // copy-out.  Reads are round trips (the kernel asks for the next tile one sample ahead: a wave waits one bus round
    // trip per tile, and the bus delivers 64-byte requests less efficiently than a DMA engine's): only the FIRST time
    // slice reads u in place -- it can start at once -- while the copy engine brings the u rows of the following slices
    // into HBM, each under the kernel of the slice before (two staging buffers).  Nothing of the transfers is exposed;
    // what remains over a device-resident run is the first slice's round trips and one launch boundary per slice
    // (a launch lasts as long as its slowest wave, slice after slice): few slices -- ACME_HOST_SLICES, default 8;
    // 1 = the whole run in place ("zero copy": 0.86 ... 0.93 x device-resident on the headline, box to box).
    // ACME_HOST_ZEROCOPY=0 keeps the fully staged pipeline below (also taken when the arrays cannot be locked).
    {
        const char *e = getenv("ACME_HOST_ZEROCOPY");
        void *du = nullptr, *dy = nullptr;
        // (not for the lane-per-instance kernels: they stream u and y sample by sample, one 8-byte access per lane
        // and sample -- over the bus that is a transaction each; the 16-lane kernels move whole tiles)
        if (!(e && e[0] == '0') && lock_u && lock_y && (nu || ny) && !use_lane_kernel(b) && !b->generic &&
            (!nu || be::host_device_pointer(&du, const_cast<double *>(u)) == 0) && (!ny || be::host_device_pointer(&dy, y) == 0)) {
            // Streamed (default for runs of 4 096 samples and more): ONE launch over the whole run; u goes into a
            // staging buffer in HBM chunk by chunk (small chunks first: the kernel starts on the first ~1 ms after the
            // call) while the kernel already runs, the host publishing after every chunk how many samples have landed
            // (KArgs::u_ready: a wave that gets ahead of the copy engine waits -- at 57 GB/s against the kernel's
            // 38 GB/s that is the start of the run only); y is written in place.  No launch boundaries, no round trips:
            // 0.99 x device-resident on the headline (301.9 against 299.3 ms).  Costs a staging buffer for all of u.
            // ACME_HOST_STREAM=0 or ACME_HOST_SLICES set: the sliced pipeline below -- also taken when a progress
            // callback is installed (one launch has no intermediate progress to report) or the buffer cannot be had.
            {
                const char *es = getenv("ACME_HOST_STREAM");
                // (rows of the staging buffer start on 128-byte boundaries and chunks are multiples of 16 samples: no
                // cache line holds both samples that have landed and samples still on their way)
                const long long Tp = (T + 15) & ~15ll;
                const size_t su_all = sizeof(double) * N * (size_t)Tp * nu;
                if (!(es && es[0] == '0') && !getenv("ACME_HOST_SLICES") && nu && T >= 4096 && b->iso_thr == 0.0 && !b->progress &&
                    b->kf->launch_stream &&
                    streamed_fits(b) && ensure_staging(b, su_all, 0, true) == ACME_OK && (b->h_u_ready || be::flag_alloc(&b->h_u_ready, &b->d_u_ready) == 0)) {
                    if (!b->copy_stream) HIPCHK(be::stream_create_nonblocking(&b->copy_stream));
                    const be::stream_t cs = b->copy_stream;
                    const bool async = be::kernels_run_async() && !getenv("ACME_HOST_STREAM_COPY_FIRST");      // (developer: the kernel only after all of u has landed)
                    volatile long long *ready = b->h_u_ready;
                    *ready = 0;
                    const auto t_begin = std::chrono::steady_clock::now();
                    int rc = ACME_OK, slot = -1;
                    if (async) rc = launch_run(b, b->d_u, (double *)dy, T, st, &slot, Tp, 0, b->d_u_ready);
                    int crc = 0;
                    // chunks: 128 samples of every row at a time (what the kernel may use lags the copy by up to one
                    // chunk, and while the copy engine is less than a chunk ahead -- it gains on the kernel by a
                    // quarter of its own pace -- every wave waits at every chunk's end: 4 096-sample chunks cost 52 ms
                    // of a 300 ms run, 1 024 15 ms, 512 9 ms, 256 4.5 ms, 128 2.5 ms; the engine is not slower for it)
                    // (round 5, with the kernel 6 % faster: 256 -- 128-sample chunks 331, 256 321 / 296, 512 318 ms on two boxes;
                    // the kernel runs ~20 % slower WHILE the copy engine works, more so with many small copies)
                    long long done = 0, chunk = 256;
                    if (const char *ec = getenv("ACME_HOST_STREAM_CHUNK")) { const long long v = atoll(ec); if (v >= 16) chunk = (v + 15) & ~15ll; }
                    while (rc == ACME_OK && done < T) {
                        const long long len = done + chunk <= T ? chunk : T - done;
                        const size_t w = sizeof(double) * (size_t)len * nu;
                        crc = be::copy2d_h2d_async(b->d_u + (size_t)done * nu, sizeof(double) * (size_t)Tp * nu, u + (size_t)done * nu,
                                                   sizeof(double) * (size_t)T * nu, w, N, cs);
                        if (crc == 0) crc = be::stream_sync(cs);
                        if (crc != 0) break;
                        done += len;
                        *ready = done;
                    }
                    *ready = T;                    // (whatever happened: no wave is left waiting)
                    const auto t_copy = std::chrono::steady_clock::now();
                    if (rc == ACME_OK && crc == 0 && !async) rc = launch_run(b, b->d_u, (double *)dy, T, st, &slot, Tp, 0, b->d_u_ready);
                    const int src = be::stream_sync(st);
                    if (getenv("ACME_HOST_STREAM_DEBUG")) {
                        const auto t_end = std::chrono::steady_clock::now();
                        fprintf(stderr, "streamed run: copies done after %.1f ms, kernel after %.1f ms\n",
                                1e3 * std::chrono::duration<double>(t_copy - t_begin).count(),
                                1e3 * std::chrono::duration<double>(t_end - t_begin).count());
                    }
                    if (rc != ACME_OK) return rc;
                    HIPCHK(crc);
                    HIPCHK(src);
                    if (b->progress) b->progress(b->progress_user, T, T);
                    return ACME_OK;
                }
            }
            long long want = 8;
            if (const char *es = getenv("ACME_HOST_SLICES")) { const long long v = atoll(es); if (v >= 1 && v <= 1024) want = v; }
            long long TS = T;
            if (nu && want > 1 && T >= 4096) {
                TS = ((T / want + CHUNK - 1) / CHUNK) * CHUNK;
                if (TS < 1024) TS = 1024;
            }
            const long long ns = (T + TS - 1) / TS;
            if (ns == 1) {
                const int rc0 = launch_run(b, (const double *)du, (double *)dy, T, st, nullptr);
                if (rc0 != ACME_OK) return rc0;
                HIPCHK(be::stream_sync(st));
                if (b->slow_stream) HIPCHK(be::stream_sync(b->slow_stream));     // (a host run returns complete)
                if (b->progress) b->progress(b->progress_user, T, T);
                return ACME_OK;
            }
            int rc = ensure_staging(b, 2 * sizeof(double) * N * (size_t)TS * nu, 0);
            if (rc == ACME_OK) rc = copy_streams(b, false);
            if (rc != ACME_OK) return rc;
            // (a loop of its own, not run_slices': slice 0 is read in place, the kernel writes y into the caller's array --
            // nothing is copied out -- and copy-in 1 is issued before the first launch, which waits for no copy)
            const Slices sl{T, TS, N, nu, 0, u, nullptr, b->d_u, nullptr, b->copy_stream, nullptr};
            int slot_prev = -1, slot = -1;
            HIPCHK(sl.copy_in(1));
            for (long long s = 0; s < ns; ++s) {
                if (s > 0) HIPCHK(be::stream_sync(sl.cs));                     // slice s of u is in HBM
                double *ys = ny ? (double *)dy + (size_t)s * TS * ny : nullptr;
                if (s == 0) rc = launch_run(b, (const double *)du, ys, sl.len(0), st, &slot, T, T);
                else rc = launch_run(b, sl.in(s), ys, sl.len(s), st, &slot, 0, T);
                if (rc != ACME_OK) return rc;
                if (s > 0) {
                    HIPCHK(be::event_sync(b->ev1[slot_prev]));                 // kernel s-1 done: its u buffer is free, ...
                    if (b->slow_stream) HIPCHK(be::stream_sync(b->slow_stream));
                    if (b->progress) b->progress(b->progress_user, s * TS, T);  // ... its y rows are in the caller's array
                    if (s + 1 < ns) HIPCHK(sl.copy_in(s + 1));
                }
                slot_prev = slot;
            }
            HIPCHK(be::stream_sync(st));
            if (b->slow_stream) HIPCHK(be::stream_sync(b->slow_stream));
            if (b->progress) b->progress(b->progress_user, T, T);
            return ACME_OK;
        }
    }
    const long long TS = staged_slice(T);
    const long long ns = (T + TS - 1) / TS;
    const size_t su = sizeof(double) * N * (size_t)TS * nu, sy = sizeof(double) * N * (size_t)TS * ny;
    int rc = ensure_staging(b, (ns > 1 ? 2 : 1) * su, (ns > 1 ? 2 : 1) * sy);
    if (rc != ACME_OK) return rc;
    if (ns == 1) {
        if (su) HIPCHK(be::copy_h2d_async(b->d_u, u, su, st));
        rc = launch_run(b, b->d_u, b->d_y, T, st, nullptr);
        if (rc != ACME_OK) return rc;
        if (b->slow_stream) HIPCHK(be::stream_sync(b->slow_stream));
        if (sy) HIPCHK(be::copy_d2h_async(y, b->d_y, sy, st));
        HIPCHK(be::stream_sync(st));
        if (b->progress) b->progress(b->progress_user, T, T);
        return ACME_OK;
    }
    if ((rc = copy_streams(b, true)) != ACME_OK) return rc;
    const Slices sl{T, TS, N, nu, ny, u, y, b->d_u, b->d_y, b->copy_stream, b->copy_stream_out};
    return run_slices(b, sl, [&](long long, const double *in, double *out, long long n, be::event_t *done) -> int {
        int slot = 0;
        const int rc_ = launch_run(b, in, out, n, st, &slot);
        *done = b->ev1[slot];
        return rc_;
    }, CopyOut{sl});      // (a progress report: the slices before are in the caller's y)
}

// run! with constant input rows (include/acme_hip.h): the varying rows come in (from the host: time slice by time slice, two
// staging buffers, copies overlapping the kernels: run_slices), the full rows of a slice are put
// together in HBM by a small kernel on the launch stream (be::launch_expand), and the run kernels see what they always see.
int acme_batch_run_const(acme_batch *b, const double *u_var, const double *u_const, unsigned long long const_mask,
                         double *y, long long T, int mem, void *stream) {
    RunGuard serial(b);
    if (!b || T < 0) return fail(ACME_ERR_INVALID, "invalid argument to acme_batch_run_const");
    if (b && b->src.armed) return fail(ACME_ERR_INVALID, "acme_batch_run_const: input rows have sources (acme_batch_set_source_*); use acme_batch_run_sources");
    const int nu = b->P.actual.nu, ny = b->P.actual.ny;
    if (nu > 64) return fail(ACME_ERR_UNSUPPORTED, "acme_batch_run_const: more than 64 input rows");
    const unsigned long long all = nu >= 64 ? ~0ull : ((1ull << nu) - 1ull);
    const_mask &= all;
    int nuv = 0;
    for (int k = 0; k < nu; ++k) nuv += (const_mask >> k & 1ull) ? 0 : 1;
    if (const_mask == 0ull) return run_impl(b, u_var, y, T, mem, stream);
    if ((nuv > 0 && T > 0 && !u_var) || !u_const || (ny > 0 && T > 0 && !y && !b->meas.on)) return fail(ACME_ERR_INVALID, "null u_var, u_const or y");
    if (mem != ACME_MEM_HOST && mem != ACME_MEM_DEVICE) return fail(ACME_ERR_INVALID, "mem must be ACME_MEM_HOST or ACME_MEM_DEVICE");
    if (T == 0) return ACME_OK;
    ON_DEVICE(b);
    be::stream_t st = (be::stream_t)stream;
    if (b->os.k > 1 || b->meas.on) return run_os(b, u_var, u_const, const_mask, y, T, mem, st);
    const size_t N = (size_t)b->N;
    int rc;
    if (mem == ACME_MEM_DEVICE) {
        rc = ensure_staging(b, sizeof(double) * N * (size_t)T * nu, 0);
        if (rc != ACME_OK) return rc;
        HIPCHK(be::launch_expand(b->d_u, u_var, u_const, const_mask, (long long)N, T, T, nu, nuv, st));
        rc = launch_run(b, b->d_u, y, T, st, nullptr);
        if (rc == ACME_OK && b->progress) b->progress(b->progress_user, T, T);
        return rc;
    }
    // a caller who keeps its arrays alive and reuses them (acme_batch_set_host_retention): u_var and y are page-locked once --
    // the slices' copies below then run at the bus's rate beside the kernels instead of through the runtime's bounce buffers
    if (!b->retain_host) { release_reg(b->reg_u); release_reg(b->reg_y); }
    else {
        (void)ensure_registered(b->reg_u, u_var, sizeof(double) * N * (size_t)T * (nuv ? nuv : 1));
        (void)ensure_registered(b->reg_y, y, sizeof(double) * N * (size_t)T * ny);
    }
    rc = os_grow(&b->d_uc, &b->cap_uc, sizeof(double) * N * (size_t)nu);
    if (rc != ACME_OK) return rc;
    HIPCHK(be::copy_h2d_async(b->d_uc, u_const, sizeof(double) * N * (size_t)nu, st));
    const long long TS = staged_slice(T);
    const long long ns = (T + TS - 1) / TS;
    const int nb = ns > 1 ? 2 : 1;
    const size_t su = sizeof(double) * N * (size_t)TS * nu, sv = sizeof(double) * N * (size_t)TS * (nuv ? nuv : 1), sy = sizeof(double) * N * (size_t)TS * ny;
    rc = ensure_staging(b, nb * su, nb * sy);
    if (rc == ACME_OK) rc = os_grow(&b->d_uv, &b->cap_uv, nb * sv);
    if (rc == ACME_OK) rc = copy_streams(b, true);
    if (rc != ACME_OK) return rc;
    const Slices sl{T, TS, N, nuv, ny, u_var, y, b->d_uv, b->d_y, b->copy_stream, b->copy_stream_out};
    // The copies run from pageable memory (nothing of the caller's arrays is kept): such a copy blocks the thread that issues
    // it, so issued from one thread the two directions take turns -- 2.9 GB each way on the headline, ~290 ms of copies for
    // 273 ms of kernels.  The y rows therefore leave through a helper thread of their own: in and out overlap each other
    // and the kernels, and the call is bound by the kernels again.
    return run_slices(b, sl, [&](long long s, const double *in, double *out, long long n, be::event_t *done) -> int {
        // (the launch stream is in order: slice s is put together behind kernel s-1 and ahead of kernel s; its buffer is the
        // one kernel s-2 read.  Kernel s done also says that expand s has read its source, `in`)
        double *full = b->d_u + (s & 1) * (N * (size_t)TS * nu);
        HIPCHK(be::launch_expand(full, in, b->d_uc, const_mask, (long long)N, n, n, nu, nuv, st));
        int slot = 0;
        const int rc_ = launch_run(b, full, out, n, st, &slot);
        *done = b->ev1[slot];
        return rc_;
    }, ThreadCopyOut{sl, b->device});
}

// run! of one batch without blocking the caller: the same call on a worker thread of the library (a
// host-buffer run drives its time-slice pipeline from there), so that ONE host thread can keep several
// batches -- one per GPU of a node -- busy at once: start them all, then wait for each.
int acme_batch_run_async(acme_batch *b, const double *u, double *y, long long T, int mem, void *stream) {
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    join_worker(b);
    if (b && b->src.armed) return fail(ACME_ERR_INVALID, "acme_batch_run_async: input rows have sources (acme_batch_set_source_*); use acme_batch_run_sources");
    return start_worker(b, [=]() { return run_impl(b, u, y, T, mem, stream); });
}

// ---- input rows generated on the device (acme_batch_set_source_*, acme_source.h) --------------------------------------------
// a per-instance parameter array in device memory; NULL stays NULL (the kind's default for every instance)
static int src_upload(const void *h, size_t bytes, const void **d) {
    *d = nullptr;
    if (!h) return ACME_OK;
    void *p = nullptr;
    HIPCHK(be::dmalloc(&p, bytes));
    const int e = be::copy_h2d(p, h, bytes);
    if (e != 0) { (void)be::dfree(p); return fail(ACME_ERR_HIP, std::string("copy of source parameters: ") + be::err_string(e)); }
    *d = p;
    return ACME_OK;
}
// the row's descriptions as the device reads them: the caller's rows numbered in row order
static int src_commit(acme_batch *b) {
    acme_batch::Sources &S = b->src;
    int v = 0;
    for (int r = 0; r < 64; ++r) S.row[r].var = S.row[r].kind == SRC_NONE ? v++ : 0;
    if (!S.d_rows) HIPCHK(be::dmalloc((void **)&S.d_rows, sizeof(S.row)));
    HIPCHK(be::copy_h2d(S.d_rows, S.row, sizeof(S.row)));
    if (!S.armed) S.clock = 0;
    return ACME_OK;
}
// kind, den (SINE, MULTISINE: f_den; TABLE: P; NOISE: hold), the arrays of the kind (host arrays of N entries, w of P; NULL =
// default; MULTISINE: f_num, phase and amp hold tones x N entries; NOISE: f_num holds the streams, tones the distribution;
// PULSE, BURST: shape holds 5 x N entries -- period, delay, rise, on, fall)
static int set_source(acme_batch *b, int row, int kind, long long den, const long long *f_num, const long long *phase,
                      const double *w, const double *amp, const double *offset, int tones = 1, const long long *shape = nullptr) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const int nu = b->P.actual.nu;
    if (nu > 64) return fail(ACME_ERR_UNSUPPORTED, "sources: more than 64 input rows");
    if (row < 0 || row >= nu) return fail(ACME_ERR_INVALID, "source: row beyond the model's inputs");
    const size_t N = (size_t)b->N;
    if (kind == SRC_MULTISINE) {
        if (tones < 1 || tones > SRC_MAX_TONES) return fail(ACME_ERR_INVALID, "multisine source: tones must be 1 ... 4");
        if (!f_num) return fail(ACME_ERR_INVALID, "multisine source: null f_num");
        if (den <= 0 || den >= (1ll << 31)) return fail(ACME_ERR_INVALID, "multisine source: f_den must be 1 ... 2^31 - 1");
        for (int k = 0; k < tones; ++k)
            for (size_t i = 0; i < N; ++i) {
                const size_t e = (size_t)k * N + i;
                if (f_num[e] < 0 || f_num[e] >= den || (phase && (phase[e] < 0 || phase[e] >= den)))
                    return fail(ACME_ERR_INVALID, "multisine source: f_num and phase must be 0 ... f_den - 1 (tone " + std::to_string(k) +
                                                      ", instance " + std::to_string(i) + ")");
                if (amp && !std::isfinite(amp[e]))
                    return fail(ACME_ERR_INVALID, "source: non-finite amp (tone " + std::to_string(k) + ", instance " + std::to_string(i) + ")");
            }
    }
    if (kind == SRC_SINE || kind == SRC_BURST) {
        const std::string what = kind == SRC_SINE ? "sine source" : "burst source";
        if (den <= 0 || den >= (1ll << 31)) return fail(ACME_ERR_INVALID, what + ": f_den must be 1 ... 2^31 - 1");
        for (size_t i = 0; i < N; ++i)
            if ((f_num && (f_num[i] < 0 || f_num[i] >= den)) || (phase && (phase[i] < 0 || phase[i] >= den)))
                return fail(ACME_ERR_INVALID, what + ": f_num and phase must be 0 ... f_den - 1 (instance " + std::to_string(i) + ")");
    }
    if (kind == SRC_PULSE || kind == SRC_BURST) {
        const std::string what = kind == SRC_PULSE ? "pulse source" : "burst source";
        if (!shape) return fail(ACME_ERR_INVALID, what + ": null shape");
        for (size_t i = 0; i < N; ++i) {
            const long long P = shape[i], delay = shape[N + i], rise = shape[2 * N + i], on = shape[3 * N + i], fall = shape[4 * N + i];
            const std::string inst = " (instance " + std::to_string(i) + ")";
            if (P < 1 || P >= (1ll << 31)) return fail(ACME_ERR_INVALID, what + ": period must be 1 ... 2^31 - 1" + inst);
            if (delay < 0 || delay >= P) return fail(ACME_ERR_INVALID, what + ": delay must be 0 ... period - 1" + inst);
            if (rise < 0 || on < 0 || fall < 0) return fail(ACME_ERR_INVALID, what + ": negative rise, on or fall" + inst);
            if (rise > P || on > P || fall > P || rise + on + fall > P)
                return fail(ACME_ERR_INVALID, what + ": rise + on + fall must not exceed the period" + inst);
        }
    }
    if (kind == SRC_TABLE) {
        if (den < 1 || den > SRC_MAX_TABLE) return fail(ACME_ERR_INVALID, "table source: P must be 1 ... 2^24");
        if (!w) return fail(ACME_ERR_INVALID, "table source: null table");
    }
    if (kind == SRC_NOISE) {
        if (tones != SRC_UNIFORM && tones != SRC_GAUSSIAN) return fail(ACME_ERR_INVALID, "noise source: dist must be ACME_NOISE_UNIFORM or ACME_NOISE_GAUSSIAN");
        if (den < 1 || den >= (1ll << 31)) return fail(ACME_ERR_INVALID, "noise source: hold must be 1 ... 2^31 - 1");
    }
    const double *amp_n = kind == SRC_MULTISINE ? nullptr : amp;       // (MULTISINE: tones x N amplitudes, checked with their tones above)
    for (size_t i = 0; i < N; ++i)
        if ((amp_n && !std::isfinite(amp_n[i])) || (offset && !std::isfinite(offset[i])))
            return fail(ACME_ERR_INVALID, "source: non-finite amp or offset (instance " + std::to_string(i) + ")");
    if (b->iso_thr > 0.0)
        return fail(ACME_ERR_UNSUPPORTED, "sources are not available while the isolation of slow instances is in force");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());          // (a launch still in flight may read the row's parameters)
    // everything is uploaded before the batch is touched: a failure leaves the row as it was
    SrcRow R{};
    R.kind = kind;
    R.den = kind == SRC_CONST ? 1 : den;
    R.tones = kind == SRC_MULTISINE || kind == SRC_NOISE ? tones : 0;
    const size_t NT = kind == SRC_MULTISINE ? N * (size_t)tones : N;
    const bool sine = kind == SRC_SINE || kind == SRC_MULTISINE || kind == SRC_BURST;
    int rc = src_upload(offset, sizeof(double) * N, (const void **)&R.off);
    if (rc == ACME_OK && kind != SRC_CONST) rc = src_upload(amp, sizeof(double) * NT, (const void **)&R.amp);
    if (rc == ACME_OK && (sine || kind == SRC_NOISE)) rc = src_upload(f_num, sizeof(long long) * NT, (const void **)&R.fnum);
    if (rc == ACME_OK && sine) rc = src_upload(phase, sizeof(long long) * NT, (const void **)&R.phase);
    if (rc == ACME_OK && kind == SRC_TABLE) rc = src_upload(w, sizeof(double) * (size_t)den, (const void **)&R.w);
    if (rc == ACME_OK && shape) rc = src_upload(shape, sizeof(long long) * 5 * N, (const void **)&R.shape);
    for (auto &e : b->os.ev) if (rc == ACME_OK && !e && be::event_create(&e) != 0) rc = fail(ACME_ERR_HIP, "hipEventCreate");      // (the host pipeline of run_os)
    if (rc != ACME_OK) {
        (void)be::dfree(const_cast<double *>(R.amp)); (void)be::dfree(const_cast<double *>(R.off)); (void)be::dfree(const_cast<double *>(R.w));
        (void)be::dfree(const_cast<long long *>(R.fnum)); (void)be::dfree(const_cast<long long *>(R.phase));
        (void)be::dfree(const_cast<long long *>(R.shape));
        return rc;
    }
    acme_batch::Sources &S = b->src;
    const bool first = S.armed == 0;
    src_release(b, row);
    S.row[row] = R;
    S.mask |= 1ull << row;
    if (kind == SRC_CONST) S.cmask |= 1ull << row;
    ++S.armed;
    if (first) S.clock = 0;
    return src_commit(b);
}

int acme_batch_set_source_const(acme_batch *b, int row, const double *offset) {
    return set_source(b, row, SRC_CONST, 1, nullptr, nullptr, nullptr, nullptr, offset);
}
int acme_batch_set_source_sine(acme_batch *b, int row, long long f_den, long long *f_num, long long *phase, const double *amp,
                               const double *offset) {
    return set_source(b, row, SRC_SINE, f_den, f_num, phase, nullptr, amp, offset);
}
int acme_batch_set_source_table(acme_batch *b, int row, const double *w, long long P, const double *amp, const double *offset) {
    return set_source(b, row, SRC_TABLE, P, nullptr, nullptr, w, amp, offset);
}
int acme_batch_set_source_multisine(acme_batch *b, int row, long long f_den, int tones, long long *f_num, long long *phase,
                                    const double *amp, const double *offset) {
    return set_source(b, row, SRC_MULTISINE, f_den, f_num, phase, nullptr, amp, offset, tones);
}

int acme_batch_set_source_noise(acme_batch *b, int row, int dist, long long hold, long long *stream, const double *amp,
                                const double *offset) {
    return set_source(b, row, SRC_NOISE, hold, stream, nullptr, nullptr, amp, offset, dist);
}

int acme_batch_set_source_pulse(acme_batch *b, int row, long long *shape, const double *amp, const double *offset) {
    return set_source(b, row, SRC_PULSE, 1, nullptr, nullptr, nullptr, amp, offset, 1, shape);
}
int acme_batch_set_source_burst(acme_batch *b, int row, long long *shape, long long f_den, long long *f_num, long long *phase,
                                const double *amp, const double *offset) {
    return set_source(b, row, SRC_BURST, f_den, f_num, phase, nullptr, amp, offset, 1, shape);
}

int acme_batch_clear_source(acme_batch *b, int row) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    if (row >= b->P.actual.nu || row >= 64) return fail(ACME_ERR_INVALID, "source: row beyond the model's inputs");
    if (!b->src.armed) return ACME_OK;
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    src_release(b, row);
    return src_commit(b);
}

int acme_batch_set_source_clock(acme_batch *b, long long n) {
    join_worker(b);
    if (!b || n < 0) return fail(ACME_ERR_INVALID, "invalid argument to acme_batch_set_source_clock");
    if (!b->src.armed) return fail(ACME_ERR_INVALID, "no input row has a source");
    b->src.clock = n;
    return ACME_OK;
}

int acme_batch_get_source_clock(acme_batch *b, long long *n) {
    join_worker(b);
    if (!b || !n) return fail(ACME_ERR_INVALID, "null argument");
    if (!b->src.armed) return fail(ACME_ERR_INVALID, "no input row has a source");
    *n = b->src.clock;
    return ACME_OK;
}

static int run_sources_impl(acme_batch *b, const double *u_var, double *y, long long T, int mem, void *stream) {
    if (!b || T < 0) return fail(ACME_ERR_INVALID, "invalid argument to acme_batch_run_sources");
    const acme_batch::Sources &S = b->src;
    if (!S.armed) return fail(ACME_ERR_INVALID, "acme_batch_run_sources: no input row has a source");
    const int nu = b->P.actual.nu, ny = b->P.actual.ny;
    if ((nu > S.armed && T > 0 && !u_var) || (ny > 0 && T > 0 && !y && !b->meas.on)) return fail(ACME_ERR_INVALID, "null u_var or y");
    if (mem != ACME_MEM_HOST && mem != ACME_MEM_DEVICE) return fail(ACME_ERR_INVALID, "mem must be ACME_MEM_HOST or ACME_MEM_DEVICE");
    if (T > LLONG_MAX - S.clock) return fail(ACME_ERR_INVALID, "acme_batch_run_sources: the source clock would overflow");
    if (T == 0) return ACME_OK;
    ON_DEVICE(b);
    return run_os(b, u_var, nullptr, 0ull, y, T, mem, (be::stream_t)stream, true);
}

int acme_batch_run_sources(acme_batch *b, const double *u_var, double *y, long long T, int mem, void *stream) {
    RunGuard serial(b);
    return run_sources_impl(b, u_var, y, T, mem, stream);
}

int acme_batch_run_sources_async(acme_batch *b, const double *u_var, double *y, long long T, int mem, void *stream) {
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    join_worker(b);
    return start_worker(b, [=]() { return run_sources_impl(b, u_var, y, T, mem, stream); });
}

// the input a source run of T samples would feed from the current clock, slice by slice: the source kernel writes into the
// caller's device array, or into one slice of scratch that is copied out (host arrays; the caller's rows staged likewise)
int acme_batch_render_sources(acme_batch *b, const double *u_var, double *u_out, long long T, int mem, void *stream) {
    RunGuard serial(b);
    if (!b || T < 0 || (T > 0 && !u_out)) return fail(ACME_ERR_INVALID, "invalid argument to acme_batch_render_sources");
    acme_batch::Sources &S = b->src;
    if (!S.armed) return fail(ACME_ERR_INVALID, "acme_batch_render_sources: no input row has a source");
    if (mem != ACME_MEM_HOST && mem != ACME_MEM_DEVICE) return fail(ACME_ERR_INVALID, "mem must be ACME_MEM_HOST or ACME_MEM_DEVICE");
    if (T > LLONG_MAX - S.clock) return fail(ACME_ERR_INVALID, "acme_batch_render_sources: the source clock would overflow");
    if (T == 0) return ACME_OK;
    ON_DEVICE(b);
    const be::stream_t st = (be::stream_t)stream;
    const int nu = b->P.actual.nu, nin = nu - S.armed;
    const size_t N = (size_t)b->N;
    const bool host = mem == ACME_MEM_HOST, var = nin > 0 && u_var;
    const long long TS = os_slice(T);
    const bool use_lds = source_lds();
    if (host) {
        HIPCHK(be::device_sync());          // (a run still in flight on another stream may use the scratch)
        int rc = os_grow(&b->os.d_base, &b->os.cap_base, sizeof(double) * N * (size_t)TS * nu);
        if (rc == ACME_OK && var) rc = ensure_staging(b, sizeof(double) * N * (size_t)TS * nin, 0);
        if (rc != ACME_OK) return rc;
    }
    for (long long t0 = 0; t0 < T; t0 += TS) {
        const long long n = T - t0 < TS ? T - t0 : TS;
        const double *uv = nullptr;
        if (var && host) {
            const size_t w = sizeof(double) * (size_t)n * nin;
            HIPCHK(be::copy2d_h2d_async(b->d_u, w, u_var + (size_t)t0 * nin, sizeof(double) * (size_t)T * nin, w, N, st));
            uv = b->d_u;
        } else if (var)
            uv = u_var + (size_t)t0 * nin;
        SrcArgs A{host ? b->os.d_base : u_out + (size_t)t0 * nu, uv, S.d_rows, (long long)N, n, host ? n : T, host ? n : T, S.clock + t0, nu, nin, 0, 0ull};
        src_plan(A, S.row, use_lds);
        HIPCHK(src_launch(A, st));
        if (host) {
            const size_t w = sizeof(double) * (size_t)n * nu;
            HIPCHK(be::copy2d_d2h_async(u_out + (size_t)t0 * nu, sizeof(double) * (size_t)T * nu, b->os.d_base, w, w, N, st));
            HIPCHK(be::stream_sync(st));          // (the scratch is the next slice's)
        }
    }
    return ACME_OK;
}

int acme_batch_set_isolation(acme_batch *b, double iters_per_sample) {
    join_worker(b);
    if (!b || !(iters_per_sample >= 0.0)) return fail(ACME_ERR_INVALID, "invalid argument to acme_batch_set_isolation");
    if (iters_per_sample > 0.0 && b->os.k > 1)
        return fail(ACME_ERR_UNSUPPORTED, "isolation of slow instances is not available on an oversampled batch");
    if (iters_per_sample > 0.0 && b->meas.on)
        return fail(ACME_ERR_UNSUPPORTED, "isolation of slow instances is not available while a measurement is armed");
    if (iters_per_sample > 0.0 && b->src.armed)
        return fail(ACME_ERR_UNSUPPORTED, "isolation of slow instances is not available while input rows have sources");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    b->iso_thr = iters_per_sample;
    if (iters_per_sample == 0.0) { b->map_fast.clear(); b->map_slow.clear(); }
    return ACME_OK;
}

int acme_oversampling_design(int factor, double *taps, int capacity) {
    if (factor < 1 || factor > OS_MAX_FACTOR) return fail(ACME_ERR_INVALID, "oversampling factor must be 1 ... 16");
    const std::vector<double> h = os_design(factor);
    if (taps && capacity >= (int)h.size()) memcpy(taps, h.data(), sizeof(double) * h.size());
    return (int)h.size();
}

int acme_batch_set_oversampling(acme_batch *b, int factor, const double *h_up, int n_up, const double *h_down, int n_down,
                                unsigned long long held_rows) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    if (factor < 1 || factor > OS_MAX_FACTOR) return fail(ACME_ERR_INVALID, "oversampling factor must be 1 ... 16");
    const int nu = b->P.actual.nu, ny = b->P.actual.ny;
    if ((h_up && (n_up < 1 || n_up > OS_MAX_TAPS)) || (h_down && (n_down < 1 || n_down > OS_MAX_TAPS)))
        return fail(ACME_ERR_INVALID, "a filter needs 1 ... 4096 taps");
    if (nu < 64 && (held_rows >> nu) != 0ull) return fail(ACME_ERR_INVALID, "held row beyond the model's inputs");
    std::vector<double> up = h_up ? std::vector<double>(h_up, h_up + n_up) : os_design(factor);
    const std::vector<double> down = h_down ? std::vector<double>(h_down, h_down + n_down) : os_design(factor);
    for (double v : up) if (!std::isfinite(v)) return fail(ACME_ERR_INVALID, "non-finite interpolation tap");
    for (double v : down) if (!std::isfinite(v)) return fail(ACME_ERR_INVALID, "non-finite decimation tap");
    if (factor > 1 && b->iso_thr > 0.0)
        return fail(ACME_ERR_UNSUPPORTED, "oversampling is not available while the isolation of slow instances is in force");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());          // (a launch still in flight may read the histories)
    acme_batch::Oversampling &O = b->os;
    (void)be::dfree(O.d_taps); (void)be::dfree(O.d_hist_u); (void)be::dfree(O.d_hist_y);
    O.d_taps = O.d_hist_u = O.d_hist_y = nullptr;
    O.k = 1;
    O.fresh = true;
    if (factor == 1) {                  // today's path: nothing of the above is used, the scratch goes
        (void)be::dfree(O.d_ou); (void)be::dfree(O.d_oy); (void)be::dfree(O.d_base);
        O.d_ou = O.d_oy = O.d_base = nullptr;
        O.cap_ou = O.cap_oy = O.cap_base = 0;
        return ACME_OK;
    }
    for (double &v : up) v *= factor;   // g = k h_up: the interpolator's passband gain 1
    O.lu = (int)up.size();
    O.ld = (int)down.size();
    O.du = (O.lu - 1) / factor;
    O.held = held_rows;
    up.insert(up.end(), down.begin(), down.end());
    HIPCHK(be::dmalloc((void **)&O.d_taps, sizeof(double) * up.size()));
    HIPCHK(be::copy_h2d(O.d_taps, up.data(), sizeof(double) * up.size()));
    HIPCHK(be::dmalloc((void **)&O.d_hist_u, sizeof(double) * (size_t)b->N * (size_t)O.du * nu));
    HIPCHK(be::dmalloc((void **)&O.d_hist_y, sizeof(double) * (size_t)b->N * (size_t)(O.ld - 1) * ny));
    for (auto &e : O.ev) if (!e) HIPCHK(be::event_create(&e));
    O.k = factor;
    return ACME_OK;
}

// the accumulators' start values and the window's start (acme_batch_set_measurement / _reset_measurement)
static int meas_zero(acme_batch *b) {
    acme_batch::Measurement &M = b->meas;
    const size_t P = (size_t)b->N * M.nrows, slot = (size_t)(4 + 2 * M.H) * P;
    // (a series: every window's slot, several slots a copy -- 32 MiB of start values at most on the host)
    const size_t W = M.W ? (size_t)M.W : 1, per = slot ? std::max<size_t>(1, std::min(W, ((size_t)4 << 20) / slot)) : 1;
    std::vector<double> a(per * slot);
    for (size_t w = 0; w < per; ++w)
        for (int k = 0; k < 4 + 2 * M.H; ++k)
            for (size_t p = 0; p < P; ++p) a[w * slot + k * P + p] = meas_init(k);
    for (size_t w = 0; slot && w < W; w += per)
        HIPCHK(be::copy_h2d(M.d_acc + w * slot, a.data(), sizeof(double) * slot * std::min(per, W - w)));
    if (M.fold) {       // (the periods stay)
        HIPCHK(meas_fold_zero(M.d_fold, P * (size_t)M.fold_pmax));
        HIPCHK(be::device_sync());
    }
    if (M.spec) {       // the sums and the carried samples (L, hop, the window and the table stay)
        HIPCHK(meas_spectrum_zero(M.d_spec_acc, P * (size_t)(M.spec_L / 2 + 1)));
        HIPCHK(meas_spectrum_zero(M.d_spec_carry, P * (size_t)M.spec_L));
        HIPCHK(be::device_sync());
    }
    if (M.cross) {      // the same of the cross-spectrum (in_row stays too)
        HIPCHK(meas_cross_zero(M.d_cross_acc, P * 4 * (size_t)(M.cross_L / 2 + 1)));
        HIPCHK(meas_cross_zero(M.d_cross_carry, P * 2 * (size_t)M.cross_L));
        HIPCHK(be::device_sync());
    }
    if (M.target) {     // the chains and the two carries (the table, which, lag and c stay)
        HIPCHK(meas_target_zero(M.d_tgt_acc, P * (size_t)MEAS_TARGET_SLOTS));
        HIPCHK(be::device_sync());
    }
    if (M.ens) {        // every slot back to the start values (the groups and the stride stay)
        const size_t plane = (size_t)M.ens_G * M.nrows * (size_t)M.ens_E;
        HIPCHK(meas_ensemble_start(M.d_ens_acc, (long long *)(M.d_ens_acc + 4 * plane), plane));
        HIPCHK(be::device_sync());
    }
    if (M.hist) {       // the counters (bins, mode and the ranges stay)
        HIPCHK(meas_hist_zero(M.d_hist_cnt, P * (size_t)(M.hist_B + 3)));
        HIPCHK(be::device_sync());
    }
    if (M.events) {     // the counters, the slots and the carries (C, E and the levels stay)
        HIPCHK(meas_events_zero(M.d_ev_cnt, M.d_ev_idx, M.d_ev_ab, M.d_ev_state, M.d_ev_prev, P, M.ev_C, M.ev_E));
        HIPCHK(be::device_sync());
    }
    if (M.wS) {         // the sections' states (the coefficients stay)
        HIPCHK(meas_weight_zero(M.d_wstate, P * 2 * (size_t)M.wS));
        HIPCHK(be::device_sync());
    }
    M.pos = 0;
    return ACME_OK;
}

// per-instance fundamentals: the instances grouped by distinct f_num, the plan (acme_measure.h) to the device.  The table's
// budget is MEAS_PI_BUDGET; ACME_MEAS_TABLE_BUDGET (bytes) in the environment overrides it (tests: chunks of one tile)
// fg: what the twiddle kernel reads per group ([F] f_num; bins: [F][H] reduced bin frequencies), grp: instance -> group
static int meas_plan_arm(acme_batch *b, const std::vector<long long> &fg, const std::vector<int> &grp, int F, long long **d_fg);
static int meas_pi_arm(acme_batch *b, const long long *f_num) {
    acme_batch::Measurement &M = b->meas;
    const size_t N = (size_t)b->N;
    std::vector<long long> fg(f_num, f_num + N);
    std::sort(fg.begin(), fg.end());
    fg.erase(std::unique(fg.begin(), fg.end()), fg.end());
    std::vector<int> grp(N);
    for (size_t i = 0; i < N; ++i) grp[i] = (int)(std::lower_bound(fg.begin(), fg.end(), f_num[i]) - fg.begin());
    M.f_num = fg.empty() ? 0 : fg[0];
    return meas_plan_arm(b, fg, grp, (int)fg.size(), &M.d_fnum_g);
}
// bins: the instances grouped by distinct tone tuple (f_num[0][i], ...) in lexicographic order; per group and bin the reduced
// frequency k = (sum_j coef[b][j] f_num[j]) mod f_den, the non-negative residue (|coef| <= 32767, f_num < 2^31: |sum| < 2^48)
static int meas_bins_arm(acme_batch *b, int tones, const long long *f_num, const int *coef) {
    acme_batch::Measurement &M = b->meas;
    const size_t N = (size_t)b->N;
    typedef std::array<long long, 4> Tup;
    std::vector<Tup> tg(N);
    for (size_t i = 0; i < N; ++i) {
        tg[i] = Tup{0, 0, 0, 0};
        for (int j = 0; j < tones; ++j) tg[i][(size_t)j] = f_num[(size_t)j * N + i];
    }
    const std::vector<Tup> all = tg;
    std::sort(tg.begin(), tg.end());
    tg.erase(std::unique(tg.begin(), tg.end()), tg.end());
    std::vector<int> grp(N);
    for (size_t i = 0; i < N; ++i) grp[i] = (int)(std::lower_bound(tg.begin(), tg.end(), all[i]) - tg.begin());
    std::vector<long long> kb(tg.size() * (size_t)M.H);
    for (size_t g = 0; g < tg.size(); ++g)
        for (int q = 0; q < M.H; ++q) {
            long long k = 0;
            for (int j = 0; j < tones; ++j) k += (long long)coef[q * tones + j] * tg[g][(size_t)j];
            k %= M.f_den;
            kb[g * (size_t)M.H + (size_t)q] = k < 0 ? k + M.f_den : k;
        }
    M.bins = true;
    return meas_plan_arm(b, kb, grp, (int)tg.size(), &M.d_kbin_g);
}
static int meas_plan_arm(acme_batch *b, const std::vector<long long> &fg, const std::vector<int> &grp, int F, long long **d_fg) {
    acme_batch::Measurement &M = b->meas;
    std::vector<int> sgrp;
    M.pi = true;
    M.F = F;
    long long budget = MEAS_PI_BUDGET;
    if (const char *e = getenv("ACME_MEAS_TABLE_BUDGET")) { const long long v = atoll(e); if (v >= 1) budget = v; }
    M.chunk = meas_pi_chunk(M.F > 0 ? M.F : 1, M.H, budget);
    meas_pi_plan(grp, b->N, M.nrows, M.F, &M.perm, &sgrp, &M.wgrp);
    auto put = [](auto **d, const auto &v) -> int {
        if (v.empty()) return ACME_OK;
        HIPCHK(be::dmalloc((void **)d, sizeof(v[0]) * v.size()));
        HIPCHK(be::copy_h2d(*d, v.data(), sizeof(v[0]) * v.size()));
        return ACME_OK;
    };
    int rc = put(d_fg, fg);
    if (rc == ACME_OK) rc = put(&M.d_perm, M.perm);
    if (rc == ACME_OK) rc = put(&M.d_sgrp, sgrp);
    if (rc == ACME_OK) rc = put(&M.d_wgrp, M.wgrp);
    return rc;
}

// spec = nullptr: off
// f_num_i != nullptr: per-instance fundamentals, host [N]
// tones > 0: bins -- f_num_i host [tones][N], coef host [harmonics][tones]
struct MeasSpec { long long start, length, f_num, f_den; int harmonics; unsigned long long rows; const long long *f_num_i;
                  int tones; const int *coef; };
static int set_measurement(acme_batch *b, const MeasSpec *spec) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const int ny = b->P.actual.ny;
    int nrows = 0;
    unsigned char row[64] = {};
    if (spec) {
        if (spec->start < 0 || spec->length < 0 || (spec->length > 0 && spec->length > LLONG_MAX - spec->start))
            return fail(ACME_ERR_INVALID, "measurement window: start and length must be >= 0");
        if (spec->f_den <= 0 || spec->f_den >= (1ll << 31)) return fail(ACME_ERR_INVALID, "measurement: f_den must be 1 ... 2^31 - 1");
        if (spec->harmonics < 0 || spec->harmonics > MEAS_MAX_H) return fail(ACME_ERR_INVALID, "measurement: harmonics must be 0 ... 32");
        if (spec->rows == 0ull && ny > 64) return fail(ACME_ERR_INVALID, "measurement: name the rows of a model with more than 64 outputs");
        if (ny < 64 && (spec->rows >> ny) != 0ull) return fail(ACME_ERR_INVALID, "measurement: row beyond the model's outputs");
        const unsigned long long rows = spec->rows ? spec->rows : ny >= 64 ? ~0ull : ((1ull << ny) - 1ull);
        for (int r = 0; r < 64 && r < ny; ++r)
            if (rows >> r & 1ull) row[nrows++] = (unsigned char)r;
        for (long long i = 0; spec->f_num_i && !spec->tones && i < b->N; ++i)
            if (spec->f_num_i[i] < 0 || spec->f_num_i[i] >= spec->f_den)
                return fail(ACME_ERR_INVALID, "measurement: f_num of instance " + std::to_string(i) + " is outside 0 ... f_den - 1");
        for (int j = 0; j < spec->tones; ++j)
            for (long long i = 0; i < b->N; ++i)
                if (spec->f_num_i[j * b->N + i] < 0 || spec->f_num_i[j * b->N + i] >= spec->f_den)
                    return fail(ACME_ERR_INVALID, "measurement: f_num of tone " + std::to_string(j) + ", instance " + std::to_string(i) +
                                                      " is outside 0 ... f_den - 1");
        for (int q = 0; spec->tones && q < spec->harmonics * spec->tones; ++q)
            if (spec->coef[q] < -32767 || spec->coef[q] > 32767)
                return fail(ACME_ERR_INVALID, "measurement: a coefficient of bin " + std::to_string(q / spec->tones) + " is outside -32767 ... 32767");
        if (b->iso_thr > 0.0)
            return fail(ACME_ERR_UNSUPPORTED, "measurements are not available while the isolation of slow instances is in force");
    }
    ON_DEVICE(b);
    HIPCHK(be::device_sync());          // (a launch still in flight may write the accumulators)
    acme_batch::Measurement &M = b->meas;
    meas_release(M);
    if (!spec) return ACME_OK;
    M.start = spec->start;
    M.length = spec->length;
    M.f_den = spec->f_den;
    M.f_num = spec->f_num % spec->f_den;
    if (M.f_num < 0) M.f_num += M.f_den;
    M.H = spec->harmonics;
    M.nrows = nrows;
    memcpy(M.row, row, sizeof(row));
    HIPCHK(be::dmalloc((void **)&M.d_acc, sizeof(double) * (size_t)(4 + 2 * M.H) * (size_t)b->N * nrows));
    if (spec->f_num_i) {
        const int rc = spec->tones ? meas_bins_arm(b, spec->tones, spec->f_num_i, spec->coef) : meas_pi_arm(b, spec->f_num_i);
        if (rc != ACME_OK) { meas_release(M); return rc; }
    }
    HIPCHK(be::dmalloc((void **)&M.d_tw, sizeof(double) * 2 * (size_t)(M.pi ? M.F : 1) * (size_t)M.H * (size_t)M.chunk));
    for (auto &e : b->os.ev) if (!e) HIPCHK(be::event_create(&e));      // (the host pipeline of run_os)
    const int rc = meas_zero(b);
    if (rc != ACME_OK) return rc;
    M.on = true;
    return ACME_OK;
}

int acme_batch_set_measurement(acme_batch *b, long long start, long long length, long long f_num, long long f_den,
                               int harmonics, unsigned long long rows) {
    const MeasSpec spec{start, length, f_num, f_den, harmonics, rows, nullptr, 0, nullptr};
    return set_measurement(b, &spec);
}

int acme_batch_set_measurement_per_instance(acme_batch *b, long long start, long long length, long long f_den,
                                            long long *f_num, int harmonics, unsigned long long rows) {
    if (b && !f_num) return fail(ACME_ERR_INVALID, "measurement: null f_num");
    const MeasSpec spec{start, length, 0, f_den, harmonics, rows, f_num, 0, nullptr};
    return set_measurement(b, &spec);
}

int acme_batch_set_measurement_bins(acme_batch *b, long long start, long long length, long long f_den, int tones, long long *f_num,
                                    int bins, const int *coef, unsigned long long rows) {
    if (b && (tones < 1 || tones > SRC_MAX_TONES)) return fail(ACME_ERR_INVALID, "measurement: tones must be 1 ... 4");
    if (b && !f_num) return fail(ACME_ERR_INVALID, "measurement: null f_num");
    if (b && (bins < 0 || bins > MEAS_MAX_H)) return fail(ACME_ERR_INVALID, "measurement: bins must be 0 ... 32");
    if (b && bins > 0 && !coef) return fail(ACME_ERR_INVALID, "measurement: null coef");
    const MeasSpec spec{start, length, 0, f_den, bins, rows, f_num, tones, coef};
    return set_measurement(b, &spec);
}

int acme_batch_get_measurement_plan(acme_batch *b, long long *n_groups, long long *chunk, long long *perm, int *wave_group) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.pi) return fail(ACME_ERR_INVALID, "no per-instance measurement is armed");
    if (n_groups) *n_groups = M.F;
    if (chunk) *chunk = M.chunk;
    if (perm && !M.perm.empty()) memcpy(perm, M.perm.data(), sizeof(long long) * M.perm.size());
    if (wave_group && !M.wgrp.empty()) memcpy(wave_group, M.wgrp.data(), sizeof(int) * M.wgrp.size());
    return ACME_OK;
}

int acme_batch_set_measurement_series(acme_batch *b, long long win, long long hop, long long windows) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement series: no measurement is armed");
    if (M.fold) return fail(ACME_ERR_UNSUPPORTED, "measurement series: the measurement has a fold (a fold per window is not supported)");
    if (M.spec) return fail(ACME_ERR_UNSUPPORTED, "measurement series: the measurement has a spectrum (a spectrum per window is not supported)");
    if (M.cross) return fail(ACME_ERR_UNSUPPORTED, "measurement series: the measurement has a cross-spectrum (a cross-spectrum per window is not supported)");
    if (M.target) return fail(ACME_ERR_UNSUPPORTED, "measurement series: the measurement has a target (a target per window is not supported)");
    if (M.ens) return fail(ACME_ERR_UNSUPPORTED, "measurement series: the measurement has an ensemble (an ensemble per window is not supported)");
    if (M.hist) return fail(ACME_ERR_UNSUPPORTED, "measurement series: the measurement has a histogram (a histogram per window is not supported)");
    if (M.events) return fail(ACME_ERR_UNSUPPORTED, "measurement series: the measurement has events (events per window are not supported)");
    if (M.length != 0) return fail(ACME_ERR_INVALID, "measurement series: the armed measurement's length must be 0 (the series sets the windows)");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement series: samples have been fed since arming (arm or reset the measurement first)");
    if (win < 1) return fail(ACME_ERR_INVALID, "measurement series: win must be >= 1");
    if (hop < win) return fail(ACME_ERR_INVALID, "measurement series: hop must be >= win");
    if (windows < 1 || windows > ACME_MAX_SERIES_WINDOWS)
        return fail(ACME_ERR_INVALID, "measurement series: windows must be 1 ... " + std::to_string((long long)ACME_MAX_SERIES_WINDOWS));
    // start + (windows - 1) hop + win within 64 bits (windows - 1 < 2^20)
    if (win > LLONG_MAX - M.start || (windows > 1 && hop > (LLONG_MAX - M.start - win) / (windows - 1)))
        return fail(ACME_ERR_INVALID, "measurement series: start + (windows - 1) hop + win overflows");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const size_t slot = sizeof(double) * (size_t)(4 + 2 * M.H) * (size_t)b->N * (size_t)M.nrows;
    if (slot && (size_t)windows > SIZE_MAX / slot)
        return fail(ACME_ERR_INVALID, "measurement series: windows: the accumulators' size overflows");
    double *acc = nullptr;
    HIPCHK(be::dmalloc((void **)&acc, slot * (size_t)windows));
    (void)be::dfree(M.d_acc);
    M.d_acc = acc;
    M.win = win;
    M.hop = hop;
    M.W = windows;
    return meas_zero(b);
}

int acme_batch_get_measurement_series(acme_batch *b, long long first, long long n, double *out, long long *counts) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.W) return fail(ACME_ERR_INVALID, "no measurement series is set");
    if (first < 0 || n < 0 || first > M.W || n > M.W - first)
        return fail(ACME_ERR_INVALID, "measurement series: first, n: windows " + std::to_string(first) + " ... beyond the series' " +
                                          std::to_string(M.W));
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const size_t P = (size_t)b->N * M.nrows, K = (size_t)(4 + 2 * M.H);
    std::vector<double> a(out ? K * P : 0);
    for (long long w = first; w < first + n; ++w) {
        const long long seen = M.pos - M.start - w * M.hop;         // (w hop < the series' span: no overflow)
        const long long c = seen < 0 ? 0 : seen < M.win ? seen : M.win;
        if (counts) counts[w - first] = c;
        if (!out || a.empty()) continue;
        HIPCHK(be::copy_d2h(a.data(), M.d_acc + (size_t)w * K * P, sizeof(double) * a.size()));
        const double inv = 1.0 / (double)c;            // (no sample measured yet: NaN and infinities)
        for (size_t p = 0; p < P; ++p) {
            double *o = out + ((size_t)(w - first) * P + p) * K;
            o[0] = a[p] * inv;
            o[1] = std::sqrt(a[P + p] * inv);
            o[2] = a[2 * P + p];
            o[3] = a[3 * P + p];
            for (int h = 0; h < M.H; ++h) {            // A_h = (2 / count) (C_h - j S_h)
                o[4 + 2 * h] = 2.0 * a[(4 + 2 * h) * P + p] * inv;
                o[5 + 2 * h] = -2.0 * a[(5 + 2 * h) * P + p] * inv;
            }
        }
    }
    return ACME_OK;
}

int acme_batch_set_measurement_fold(acme_batch *b, long long period, long long *period_i) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement fold: no measurement is armed");
    if (M.W) return fail(ACME_ERR_UNSUPPORTED, "measurement fold: the measurement has a series of windows (a fold per window is not supported)");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement fold: samples have been fed since arming (arm or reset the measurement first)");
    const std::string range = " outside 1 ... " + std::to_string(MEAS_MAX_FOLD_PERIOD);
    if (!period_i && (period < 1 || period > MEAS_MAX_FOLD_PERIOD)) return fail(ACME_ERR_INVALID, "measurement fold: period is" + range);
    std::vector<long long> per((size_t)b->N, period);
    long long pmax = 0;
    for (long long i = 0; i < b->N; ++i) {
        if (period_i) per[(size_t)i] = period_i[i];
        if (per[(size_t)i] < 1 || per[(size_t)i] > MEAS_MAX_FOLD_PERIOD)
            return fail(ACME_ERR_INVALID, "measurement fold: period_i of instance " + std::to_string(i) + " is" + range);
        pmax = std::max(pmax, per[(size_t)i]);
    }
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    (void)be::dfree(M.d_fold_per); (void)be::dfree(M.d_fold);       // (a fold set again replaces the earlier one)
    M.d_fold_per = nullptr;
    M.d_fold = nullptr;
    M.fold = false;
    const size_t count = (size_t)b->N * (size_t)M.nrows * (size_t)pmax;
    HIPCHK(be::dmalloc((void **)&M.d_fold_per, sizeof(long long) * per.size()));
    HIPCHK(be::dmalloc((void **)&M.d_fold, sizeof(double) * count));
    HIPCHK(be::copy_h2d(M.d_fold_per, per.data(), sizeof(long long) * per.size()));
    HIPCHK(meas_fold_zero(M.d_fold, count));
    HIPCHK(be::device_sync());
    M.fold_per = std::move(per);
    M.fold_pmax = pmax;
    M.fold = true;
    return ACME_OK;
}

static int get_measurement_fold(acme_batch *b, double *out, long long *period, long long *count, bool sums) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.fold) return fail(ACME_ERR_INVALID, "no measurement fold is set");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const long long end = M.length ? M.start + M.length : LLONG_MAX;
    const long long cnt = (M.pos < end ? M.pos : end) - M.start, c = cnt > 0 ? cnt : 0;
    if (count) *count = c;
    if (period) memcpy(period, M.fold_per.data(), sizeof(long long) * M.fold_per.size());
    if (!out) return ACME_OK;
    const size_t pm = (size_t)M.fold_pmax, pairs = (size_t)b->N * M.nrows;
    if (pairs) HIPCHK(be::copy_d2h(out, M.d_fold, sizeof(double) * pairs * pm));     // (the accumulators' layout is the result's)
    for (size_t p = 0; p < pairs; ++p) {
        const long long P = M.fold_per[p / (size_t)M.nrows];
        double *o = out + p * pm;
        for (long long s = 0; s < M.fold_pmax; ++s) {
            const long long cs = s < P && c > s ? (c - s - 1) / P + 1 : 0;      // the samples slot s has received
            o[s] = cs == 0 ? NAN : sums ? o[s] : o[s] / (double)cs;
        }
    }
    return ACME_OK;
}

int acme_batch_get_measurement_fold(acme_batch *b, double *out, long long *period, long long *count) {
    return get_measurement_fold(b, out, period, count, false);
}

int acme_batch_get_measurement_fold_sums(acme_batch *b, double *out) {
    if (b && !out) return fail(ACME_ERR_INVALID, "measurement fold sums: out is null");
    return get_measurement_fold(b, out, nullptr, nullptr, true);
}

// the spectrum's twiddles: (cos, -sin)(2 pi k / L), k < L / 2, each component the extended-precision value rounded once;
// exactly (1, 0) at k = 0 and (0, -1) at k = L / 4
static std::vector<double> spectrum_table(long long L) {
    std::vector<double> tw((size_t)L);
    const long double two_pi = 2.0L * acosl(-1.0L);
    for (long long k = 0; k < L / 2; ++k) {
        const long double th = two_pi * (long double)k / (long double)L;
        tw[(size_t)(2 * k)] = (double)cosl(th);
        tw[(size_t)(2 * k + 1)] = (double)-sinl(th);
    }
    tw[0] = 1.0; tw[1] = 0.0;
    tw[(size_t)(L / 2)] = 0.0; tw[(size_t)(L / 2 + 1)] = -1.0;
    return tw;
}

int acme_batch_set_measurement_spectrum(acme_batch *b, long long L, long long hop, const double *w) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement spectrum: no measurement is armed");
    if (M.W) return fail(ACME_ERR_UNSUPPORTED, "measurement spectrum: the measurement has a series of windows (a spectrum per window is not supported)");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement spectrum: samples have been fed since arming (arm or reset the measurement first)");
    if (L < MEAS_MIN_SPECTRUM || L > MEAS_MAX_SPECTRUM || (L & (L - 1)) != 0)
        return fail(ACME_ERR_INVALID, "measurement spectrum: L must be a power of two, " + std::to_string(MEAS_MIN_SPECTRUM) + " ... " +
                                          std::to_string(MEAS_MAX_SPECTRUM));
    if (hop < 1 || hop > L) return fail(ACME_ERR_INVALID, "measurement spectrum: hop is outside 1 ... L");
    std::vector<double> win((size_t)L, 1.0);
    for (long long j = 0; w && j < L; ++j) {
        if (!std::isfinite(w[j])) return fail(ACME_ERR_INVALID, "measurement spectrum: w[" + std::to_string(j) + "] is not finite");
        win[(size_t)j] = w[j];
    }
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    (void)be::dfree(M.d_spec_w); (void)be::dfree(M.d_spec_tw); (void)be::dfree(M.d_spec_acc); (void)be::dfree(M.d_spec_carry);
    M.d_spec_w = M.d_spec_tw = M.d_spec_acc = M.d_spec_carry = nullptr;     // (a spectrum set again replaces the earlier one)
    M.spec = false;
    std::vector<double> tw = spectrum_table(L);
    const size_t pairs = (size_t)b->N * (size_t)M.nrows;
    HIPCHK(be::dmalloc((void **)&M.d_spec_w, sizeof(double) * (size_t)L));
    HIPCHK(be::dmalloc((void **)&M.d_spec_tw, sizeof(double) * (size_t)L));
    HIPCHK(be::dmalloc((void **)&M.d_spec_acc, sizeof(double) * pairs * (size_t)(L / 2 + 1)));
    HIPCHK(be::dmalloc((void **)&M.d_spec_carry, sizeof(double) * pairs * (size_t)L));
    HIPCHK(be::copy_h2d(M.d_spec_w, win.data(), sizeof(double) * (size_t)L));
    HIPCHK(be::copy_h2d(M.d_spec_tw, tw.data(), sizeof(double) * (size_t)L));
    HIPCHK(meas_spectrum_zero(M.d_spec_acc, pairs * (size_t)(L / 2 + 1)));
    HIPCHK(meas_spectrum_zero(M.d_spec_carry, pairs * (size_t)L));
    HIPCHK(be::device_sync());
    M.spec_w = std::move(win);
    M.spec_tw = std::move(tw);
    M.spec_L = L;
    M.spec_hop = hop;
    M.spec = true;
    return ACME_OK;
}

static int get_measurement_spectrum(acme_batch *b, double *out, long long *segments, long long *count, bool sums) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.spec) return fail(ACME_ERR_INVALID, "no measurement spectrum is set");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const long long end = M.length ? M.start + M.length : LLONG_MAX;
    const long long cnt = (M.pos < end ? M.pos : end) - M.start, c = cnt > 0 ? cnt : 0;
    const long long S = c >= M.spec_L ? (c - M.spec_L) / M.spec_hop + 1 : 0;
    if (count) *count = c;
    if (segments) *segments = S;
    if (!out) return ACME_OK;
    const size_t total = (size_t)b->N * M.nrows * (size_t)(M.spec_L / 2 + 1);
    if (total) HIPCHK(be::copy_d2h(out, M.d_spec_acc, sizeof(double) * total));     // (the accumulators' layout is the result's)
    for (size_t k = 0; k < total; ++k) out[k] = S == 0 ? NAN : sums ? out[k] : out[k] / (double)S;
    return ACME_OK;
}

int acme_batch_get_measurement_spectrum(acme_batch *b, double *out, long long *segments, long long *count) {
    return get_measurement_spectrum(b, out, segments, count, false);
}

int acme_batch_get_measurement_spectrum_sums(acme_batch *b, double *out) {
    if (b && !out) return fail(ACME_ERR_INVALID, "measurement spectrum sums: out is null");
    return get_measurement_spectrum(b, out, nullptr, nullptr, true);
}

int acme_batch_get_measurement_spectrum_table(acme_batch *b, double *w, double *tw) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.spec) return fail(ACME_ERR_INVALID, "no measurement spectrum is set");
    if (w) memcpy(w, M.spec_w.data(), sizeof(double) * M.spec_w.size());
    if (tw) memcpy(tw, M.spec_tw.data(), sizeof(double) * M.spec_tw.size());
    return ACME_OK;
}

int acme_batch_set_measurement_cross(acme_batch *b, int in_row, long long L, long long hop, const double *w) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement cross: no measurement is armed");
    if (M.W) return fail(ACME_ERR_UNSUPPORTED, "measurement cross: the measurement has a series of windows (a cross-spectrum per window is not supported)");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement cross: samples have been fed since arming (arm or reset the measurement first)");
    const int nu = b->P.actual.nu;
    if (nu == 0) return fail(ACME_ERR_INVALID, "measurement cross: the model has no input row (nu = 0)");
    if (in_row < 0 || in_row >= nu) return fail(ACME_ERR_INVALID, "measurement cross: in_row is outside 0 ... nu - 1 = " + std::to_string(nu - 1));
    if (L < MEAS_MIN_SPECTRUM || L > MEAS_MAX_SPECTRUM || (L & (L - 1)) != 0)
        return fail(ACME_ERR_INVALID, "measurement cross: L must be a power of two, " + std::to_string(MEAS_MIN_SPECTRUM) + " ... " +
                                          std::to_string(MEAS_MAX_SPECTRUM));
    if (hop < 1 || hop > L) return fail(ACME_ERR_INVALID, "measurement cross: hop is outside 1 ... L");
    std::vector<double> win((size_t)L, 1.0);
    for (long long j = 0; w && j < L; ++j) {
        if (!std::isfinite(w[j])) return fail(ACME_ERR_INVALID, "measurement cross: w[" + std::to_string(j) + "] is not finite");
        win[(size_t)j] = w[j];
    }
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    (void)be::dfree(M.d_cross_w); (void)be::dfree(M.d_cross_tw); (void)be::dfree(M.d_cross_acc); (void)be::dfree(M.d_cross_carry);
    M.d_cross_w = M.d_cross_tw = M.d_cross_acc = M.d_cross_carry = nullptr; // (a cross-spectrum set again replaces the earlier one)
    M.cross = false;
    std::vector<double> tw = spectrum_table(L);
    const size_t pairs = (size_t)b->N * (size_t)M.nrows;
    HIPCHK(be::dmalloc((void **)&M.d_cross_w, sizeof(double) * (size_t)L));
    HIPCHK(be::dmalloc((void **)&M.d_cross_tw, sizeof(double) * (size_t)L));
    HIPCHK(be::dmalloc((void **)&M.d_cross_acc, sizeof(double) * pairs * 4 * (size_t)(L / 2 + 1)));
    HIPCHK(be::dmalloc((void **)&M.d_cross_carry, sizeof(double) * pairs * 2 * (size_t)L));
    HIPCHK(be::copy_h2d(M.d_cross_w, win.data(), sizeof(double) * (size_t)L));
    HIPCHK(be::copy_h2d(M.d_cross_tw, tw.data(), sizeof(double) * (size_t)L));
    HIPCHK(meas_cross_zero(M.d_cross_acc, pairs * 4 * (size_t)(L / 2 + 1)));
    HIPCHK(meas_cross_zero(M.d_cross_carry, pairs * 2 * (size_t)L));
    HIPCHK(be::device_sync());
    M.cross_w = std::move(win);
    M.cross_tw = std::move(tw);
    M.cross_L = L;
    M.cross_hop = hop;
    M.cross_in = in_row;
    M.cross = true;
    return ACME_OK;
}

static int get_measurement_cross(acme_batch *b, double *out, long long *segments, long long *count, bool sums) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.cross) return fail(ACME_ERR_INVALID, "no measurement cross-spectrum is set");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const long long end = M.length ? M.start + M.length : LLONG_MAX;
    const long long cnt = (M.pos < end ? M.pos : end) - M.start, c = cnt > 0 ? cnt : 0;
    const long long S = c >= M.cross_L ? (c - M.cross_L) / M.cross_hop + 1 : 0;
    if (count) *count = c;
    if (segments) *segments = S;
    if (!out) return ACME_OK;
    const size_t total = (size_t)b->N * M.nrows * 4 * (size_t)(M.cross_L / 2 + 1);
    if (total) HIPCHK(be::copy_d2h(out, M.d_cross_acc, sizeof(double) * total));    // (the accumulators' layout is the result's)
    for (size_t k = 0; k < total; ++k) out[k] = S == 0 ? NAN : sums ? out[k] : out[k] / (double)S;
    return ACME_OK;
}

int acme_batch_get_measurement_cross(acme_batch *b, double *out, long long *segments, long long *count) {
    return get_measurement_cross(b, out, segments, count, false);
}

int acme_batch_get_measurement_cross_sums(acme_batch *b, double *out) {
    if (b && !out) return fail(ACME_ERR_INVALID, "measurement cross sums: out is null");
    return get_measurement_cross(b, out, nullptr, nullptr, true);
}

int acme_batch_get_measurement_cross_table(acme_batch *b, double *w, double *tw) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.cross) return fail(ACME_ERR_INVALID, "no measurement cross-spectrum is set");
    if (w) memcpy(w, M.cross_w.data(), sizeof(double) * M.cross_w.size());
    if (tw) memcpy(tw, M.cross_tw.data(), sizeof(double) * M.cross_tw.size());
    return ACME_OK;
}

int acme_batch_set_measurement_target(acme_batch *b, const double *t, long long K, long long P, const int *which, long long *lag,
                                      double preemph) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement target: no measurement is armed");
    if (M.W) return fail(ACME_ERR_UNSUPPORTED, "measurement target: the measurement has a series of windows (a target per window is not supported)");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement target: samples have been fed since arming (arm or reset the measurement first)");
    if (!t) return fail(ACME_ERR_INVALID, "measurement target: t is null");
    if (K < 1 || K > MEAS_MAX_TARGETS) return fail(ACME_ERR_INVALID, "measurement target: K is outside 1 ... " + std::to_string(MEAS_MAX_TARGETS));
    if (P < 1) return fail(ACME_ERR_INVALID, "measurement target: P must be >= 1");
    const long long per = K * (long long)(M.nrows > 0 ? M.nrows : 1);       // (<= 64 x 64)
    if (P > (long long)ACME_MAX_SOURCE_TABLE / per)
        return fail(ACME_ERR_INVALID, "measurement target: K nrows P exceeds " + std::to_string((long long)ACME_MAX_SOURCE_TABLE));
    if (!(preemph >= 0.0 && preemph < 1.0)) return fail(ACME_ERR_INVALID, "measurement target: preemph is outside 0 <= c < 1");
    const size_t total = (size_t)K * (size_t)M.nrows * (size_t)P, N = (size_t)b->N, pairs = N * (size_t)M.nrows;
    for (size_t k = 0; k < total; ++k)
        if (!std::isfinite(t[k])) return fail(ACME_ERR_INVALID, "measurement target: t[" + std::to_string(k) + "] is not finite");
    std::vector<int> wh(N, 0), wuni;
    std::vector<long long> lg(N, 0);
    for (size_t i = 0; i < N; ++i) {
        if (which) wh[i] = which[i];
        if (lag) lg[i] = lag[i];
        if (wh[i] < 0 || wh[i] >= K)
            return fail(ACME_ERR_INVALID, "measurement target: which of instance " + std::to_string(i) + " is outside 0 ... K - 1 = " + std::to_string(K - 1));
        if (lg[i] < 0 || lg[i] >= P)
            return fail(ACME_ERR_INVALID, "measurement target: lag of instance " + std::to_string(i) + " is outside 0 ... P - 1 = " + std::to_string(P - 1));
    }
    meas_target_plan(wh.data(), lg.data(), b->N, M.nrows, &wuni);
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    (void)be::dfree(M.d_tgt); (void)be::dfree(M.d_tgt_which); (void)be::dfree(M.d_tgt_wuni); (void)be::dfree(M.d_tgt_lag); (void)be::dfree(M.d_tgt_acc);
    M.d_tgt = M.d_tgt_acc = nullptr;    // (a target set again replaces the earlier one)
    M.d_tgt_which = M.d_tgt_wuni = nullptr;
    M.d_tgt_lag = nullptr;
    M.target = false;
    HIPCHK(be::dmalloc((void **)&M.d_tgt, sizeof(double) * std::max<size_t>(total, 1)));
    HIPCHK(be::dmalloc((void **)&M.d_tgt_which, sizeof(int) * std::max<size_t>(N, 1)));
    HIPCHK(be::dmalloc((void **)&M.d_tgt_lag, sizeof(long long) * std::max<size_t>(N, 1)));
    HIPCHK(be::dmalloc((void **)&M.d_tgt_wuni, sizeof(int) * std::max<size_t>(wuni.size(), 1)));
    HIPCHK(be::dmalloc((void **)&M.d_tgt_acc, sizeof(double) * std::max<size_t>(pairs * MEAS_TARGET_SLOTS, 1)));
    if (total) HIPCHK(be::copy_h2d(M.d_tgt, t, sizeof(double) * total));
    if (N) HIPCHK(be::copy_h2d(M.d_tgt_which, wh.data(), sizeof(int) * N));
    if (N) HIPCHK(be::copy_h2d(M.d_tgt_lag, lg.data(), sizeof(long long) * N));
    if (!wuni.empty()) HIPCHK(be::copy_h2d(M.d_tgt_wuni, wuni.data(), sizeof(int) * wuni.size()));
    HIPCHK(meas_target_zero(M.d_tgt_acc, pairs * MEAS_TARGET_SLOTS));
    HIPCHK(be::device_sync());
    M.tgt_K = K;
    M.tgt_P = P;
    M.tgt_c = preemph;
    M.target = true;
    return ACME_OK;
}

int acme_batch_get_measurement_target(acme_batch *b, double *out, long long *count) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.target) return fail(ACME_ERR_INVALID, "no measurement target is set");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const long long end = M.length ? M.start + M.length : LLONG_MAX;
    const long long cnt = (M.pos < end ? M.pos : end) - M.start;
    if (count) *count = cnt > 0 ? cnt : 0;
    if (!out) return ACME_OK;
    const size_t pairs = (size_t)b->N * M.nrows;
    std::vector<double> a(pairs * MEAS_TARGET_SLOTS);
    if (!a.empty()) HIPCHK(be::copy_d2h(a.data(), M.d_tgt_acc, sizeof(double) * a.size()));
    for (size_t p = 0; p < pairs; ++p)
        for (int k = 0; k < 7; ++k) out[p * 7 + k] = a[(size_t)k * pairs + p];
    return ACME_OK;
}

int acme_batch_set_measurement_weighting(acme_batch *b, const double *sos, int S) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement weighting: no measurement is armed");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement weighting: samples have been fed since arming (arm or reset the measurement first)");
    if (!sos) return fail(ACME_ERR_INVALID, "measurement weighting: sos is null");
    if (S < 1 || S > MEAS_MAX_WEIGHT_SECTIONS)
        return fail(ACME_ERR_INVALID, "measurement weighting: S is outside 1 ... " + std::to_string(MEAS_MAX_WEIGHT_SECTIONS));
    for (int k = 0; k < 5 * S; ++k)
        if (!std::isfinite(sos[k]))
            return fail(ACME_ERR_INVALID, "measurement weighting: sos[" + std::to_string(k / 5) + "][" + std::to_string(k % 5) + "] is not finite");
    const size_t states = (size_t)b->N * M.nrows * 2 * (size_t)S;
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    (void)be::dfree(M.d_wstate);        // (a weighting set again replaces the earlier one)
    M.d_wstate = nullptr;
    M.wS = 0;
    HIPCHK(be::dmalloc((void **)&M.d_wstate, sizeof(double) * std::max<size_t>(states, 1)));
    HIPCHK(meas_weight_zero(M.d_wstate, states));
    HIPCHK(be::device_sync());
    memset(M.wsos, 0, sizeof(M.wsos));
    memcpy(M.wsos, sos, sizeof(double) * 5 * (size_t)S);
    M.wS = S;
    return ACME_OK;
}

int acme_batch_get_measurement_weighting(acme_batch *b, double *sos, int *S) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.wS) return fail(ACME_ERR_INVALID, "no measurement weighting is set");
    if (S) *S = M.wS;
    if (sos) memcpy(sos, M.wsos, sizeof(M.wsos));
    return ACME_OK;
}

int acme_batch_set_measurement_ensemble(acme_batch *b, const int *group, int G, long long stride) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement ensemble: no measurement is armed");
    if (M.W) return fail(ACME_ERR_UNSUPPORTED, "measurement ensemble: the measurement has a series of windows (an ensemble per window is not supported)");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement ensemble: samples have been fed since arming (arm or reset the measurement first)");
    if (M.length <= 0) return fail(ACME_ERR_INVALID, "measurement ensemble: the armed measurement's window must be bounded (length > 0)");
    if (G < 1) return fail(ACME_ERR_INVALID, "measurement ensemble: G must be >= 1");
    if (stride < 1) return fail(ACME_ERR_INVALID, "measurement ensemble: stride must be >= 1");
    const long long E = (M.length - 1) / stride + 1, GR = (long long)G * (long long)M.nrows;
    if (GR > 0 && E > MEAS_MAX_ENSEMBLE / GR)
        return fail(ACME_ERR_INVALID, "measurement ensemble: G nrows E exceeds " + std::to_string(MEAS_MAX_ENSEMBLE));
    for (long long i = 0; group && i < b->N; ++i)
        if (group[i] < -1 || group[i] >= G)
            return fail(ACME_ERR_INVALID, "measurement ensemble: group of instance " + std::to_string(i) + " is outside -1 ... G - 1 = " + std::to_string(G - 1));
    std::vector<int> member;
    std::vector<long long> off;
    meas_ensemble_plan(group, b->N, G, &member, &off);
    const size_t plane = (size_t)GR * (size_t)E;
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    (void)be::dfree(M.d_ens_member); (void)be::dfree(M.d_ens_off); (void)be::dfree(M.d_ens_acc);
    M.d_ens_member = nullptr;           // (an ensemble set again replaces the earlier one)
    M.d_ens_off = nullptr;
    M.d_ens_acc = nullptr;
    M.ens = false;
    HIPCHK(be::dmalloc((void **)&M.d_ens_member, sizeof(int) * std::max<size_t>(member.size(), 1)));
    HIPCHK(be::dmalloc((void **)&M.d_ens_off, sizeof(long long) * off.size()));
    HIPCHK(be::dmalloc((void **)&M.d_ens_acc, sizeof(double) * std::max<size_t>(6 * plane, 1)));
    if (!member.empty()) HIPCHK(be::copy_h2d(M.d_ens_member, member.data(), sizeof(int) * member.size()));
    HIPCHK(be::copy_h2d(M.d_ens_off, off.data(), sizeof(long long) * off.size()));
    HIPCHK(meas_ensemble_start(M.d_ens_acc, (long long *)(M.d_ens_acc + 4 * plane), plane));
    HIPCHK(be::device_sync());
    M.ens_G = G;
    M.ens_stride = stride;
    M.ens_E = E;
    M.ens_off = off;
    M.ens = true;
    return ACME_OK;
}

int acme_batch_get_measurement_ensemble(acme_batch *b, double *out, long long *arg, long long *members, long long *filled) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.ens) return fail(ACME_ERR_INVALID, "no measurement ensemble is set");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const long long end = M.start + M.length;
    const long long cnt = (M.pos < end ? M.pos : end) - M.start;
    if (filled) *filled = cnt > 0 ? (cnt - 1) / M.ens_stride + 1 : 0;
    for (int g = 0; members && g < M.ens_G; ++g) members[g] = M.ens_off[(size_t)g + 1] - M.ens_off[(size_t)g];
    const size_t GR = (size_t)M.ens_G * M.nrows, E = (size_t)M.ens_E, plane = GR * E;
    if (out) {
        std::vector<double> a(4 * plane);
        if (!a.empty()) HIPCHK(be::copy_d2h(a.data(), M.d_ens_acc, sizeof(double) * a.size()));
        for (size_t q = 0; q < plane; ++q)
            for (int k = 0; k < 4; ++k) out[q * 4 + k] = a[(size_t)k * plane + q];
    }
    if (arg) {
        std::vector<long long> a(2 * plane);
        if (!a.empty()) HIPCHK(be::copy_d2h(a.data(), M.d_ens_acc + 4 * plane, sizeof(long long) * a.size()));
        for (size_t q = 0; q < plane; ++q)
            for (int k = 0; k < 2; ++k) arg[q * 2 + k] = a[(size_t)k * plane + q];
    }
    return ACME_OK;
}

int acme_batch_set_measurement_histogram(acme_batch *b, int bins, int mode, double lo, double hi, const double *lo_i, const double *hi_i) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement histogram: no measurement is armed");
    if (M.W) return fail(ACME_ERR_UNSUPPORTED, "measurement histogram: the measurement has a series of windows (a histogram per window is not supported)");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement histogram: samples have been fed since arming (arm or reset the measurement first)");
    if (bins < 1 || bins > MEAS_MAX_HIST_BINS)
        return fail(ACME_ERR_INVALID, "measurement histogram: bins is outside 1 ... " + std::to_string(MEAS_MAX_HIST_BINS));
    if (mode != MEAS_HIST_SIGNED && mode != MEAS_HIST_ABS)
        return fail(ACME_ERR_INVALID, "measurement histogram: mode must be ACME_HIST_SIGNED (0) or ACME_HIST_ABS (1)");
    if ((lo_i == nullptr) != (hi_i == nullptr))
        return fail(ACME_ERR_INVALID, std::string("measurement histogram: ") + (lo_i ? "hi_i" : "lo_i") + " is NULL beside the other array (both or neither)");
    const long long PR = b->N * (long long)M.nrows;
    if (PR > 0 && (long long)(bins + 3) > MEAS_MAX_HISTOGRAM / PR)
        return fail(ACME_ERR_INVALID, "measurement histogram: N nrows (B + 3) exceeds " + std::to_string(MEAS_MAX_HISTOGRAM));
    std::vector<double> range((size_t)b->N * 3);
    for (long long i = 0; i < b->N; ++i) {      // the scale, formed once: two roundings
        const double l = lo_i ? lo_i[i] : lo, h = hi_i ? hi_i[i] : hi;
        const std::string at = lo_i ? " of instance " + std::to_string(i) : std::string();
        const char *ln = lo_i ? "lo_i" : "lo", *hn = lo_i ? "hi_i" : "hi";
        if (!std::isfinite(l)) return fail(ACME_ERR_INVALID, std::string("measurement histogram: ") + ln + at + " is not finite");
        if (!std::isfinite(h)) return fail(ACME_ERR_INVALID, std::string("measurement histogram: ") + hn + at + " is not finite");
        if (l >= h) return fail(ACME_ERR_INVALID, std::string("measurement histogram: ") + ln + " >= " + hn + at);
        double d, s;
        meas_hist_scale(l, h, bins, &d, &s);
        if (!std::isfinite(d)) return fail(ACME_ERR_INVALID, std::string("measurement histogram: ") + hn + " - " + ln + at + " overflows");
        if (!std::isfinite(s)) return fail(ACME_ERR_INVALID, std::string("measurement histogram: bins / (") + hn + " - " + ln + ")" + at + " overflows");
        range[(size_t)i * 3] = l; range[(size_t)i * 3 + 1] = h; range[(size_t)i * 3 + 2] = s;
    }
    const size_t count = (size_t)PR * (size_t)(bins + 3);
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    (void)be::dfree(M.d_hist_cnt); (void)be::dfree(M.d_hist_range);     // (a histogram set again replaces the earlier one)
    M.d_hist_cnt = nullptr;
    M.d_hist_range = nullptr;
    M.hist = false;
    HIPCHK(be::dmalloc((void **)&M.d_hist_cnt, sizeof(long long) * std::max<size_t>(count, 1)));
    HIPCHK(be::dmalloc((void **)&M.d_hist_range, sizeof(double) * std::max<size_t>(range.size(), 1)));
    if (!range.empty()) HIPCHK(be::copy_h2d(M.d_hist_range, range.data(), sizeof(double) * range.size()));
    HIPCHK(meas_hist_zero(M.d_hist_cnt, count));
    HIPCHK(be::device_sync());
    M.hist_range = std::move(range);
    M.hist_B = bins;
    M.hist_mode = mode;
    M.hist = true;
    return ACME_OK;
}

int acme_batch_get_measurement_histogram(acme_batch *b, long long *counts, double *range, long long *count) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.hist) return fail(ACME_ERR_INVALID, "no measurement histogram is set");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const long long end = M.length ? M.start + M.length : LLONG_MAX;
    const long long cnt = (M.pos < end ? M.pos : end) - M.start;
    if (count) *count = cnt > 0 ? cnt : 0;
    if (range && !M.hist_range.empty()) memcpy(range, M.hist_range.data(), sizeof(double) * M.hist_range.size());
    const size_t n = (size_t)b->N * M.nrows * (size_t)(M.hist_B + 3);
    if (counts && n) HIPCHK(be::copy_d2h(counts, M.d_hist_cnt, sizeof(long long) * n));     // (the counters' layout is the result's)
    return ACME_OK;
}

int acme_batch_set_measurement_events(acme_batch *b, int C, const double *lo, const double *hi, int E) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "measurement events: no measurement is armed");
    if (M.W) return fail(ACME_ERR_UNSUPPORTED, "measurement events: the measurement has a series of windows (events per window are not supported)");
    if (M.pos != 0) return fail(ACME_ERR_INVALID, "measurement events: samples have been fed since arming (arm or reset the measurement first)");
    if (C < 1 || C > MEAS_MAX_EVENT_LEVELS)
        return fail(ACME_ERR_INVALID, "measurement events: C is outside 1 ... " + std::to_string(MEAS_MAX_EVENT_LEVELS));
    if (E < 0 || E > MEAS_MAX_EVENT_SLOTS)
        return fail(ACME_ERR_INVALID, "measurement events: E is outside 0 ... " + std::to_string(MEAS_MAX_EVENT_SLOTS));
    if (!lo) return fail(ACME_ERR_INVALID, "measurement events: lo is NULL");
    if (!hi) return fail(ACME_ERR_INVALID, "measurement events: hi is NULL");
    const long long PR = b->N * (long long)M.nrows;
    if (PR > 0 && (long long)C * (E + 1) > MEAS_MAX_EVENTS / PR)
        return fail(ACME_ERR_INVALID, "measurement events: N nrows C (E + 1) exceeds " + std::to_string(MEAS_MAX_EVENTS));
    const size_t CN = (size_t)C * (size_t)b->N;
    for (int c = 0; c < C; ++c)
        for (long long i = 0; i < b->N; ++i) {
            const double l = lo[c * b->N + i], h = hi[c * b->N + i];
            const std::string at = " of level " + std::to_string(c) + ", instance " + std::to_string(i);
            if (!std::isfinite(l)) return fail(ACME_ERR_INVALID, "measurement events: lo" + at + " is not finite");
            if (!std::isfinite(h)) return fail(ACME_ERR_INVALID, "measurement events: hi" + at + " is not finite");
            if (l > h) return fail(ACME_ERR_INVALID, "measurement events: lo > hi" + at);
        }
    std::vector<double> lev(2 * CN);
    if (CN) { memcpy(lev.data(), lo, sizeof(double) * CN); memcpy(lev.data() + CN, hi, sizeof(double) * CN); }
    const size_t tri = (size_t)PR * (size_t)C, rec = tri * 2 * (size_t)(E + 1);
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    (void)be::dfree(M.d_ev_lev); (void)be::dfree(M.d_ev_cnt); (void)be::dfree(M.d_ev_idx); (void)be::dfree(M.d_ev_ab);    // (events set again replace the earlier ones)
    (void)be::dfree(M.d_ev_state); (void)be::dfree(M.d_ev_prev);
    M.d_ev_lev = M.d_ev_ab = M.d_ev_prev = nullptr;
    M.d_ev_cnt = M.d_ev_idx = nullptr;
    M.d_ev_state = nullptr;
    M.events = false;
    HIPCHK(be::dmalloc((void **)&M.d_ev_lev, sizeof(double) * std::max<size_t>(lev.size(), 1)));
    HIPCHK(be::dmalloc((void **)&M.d_ev_cnt, sizeof(long long) * std::max<size_t>(tri * 5, 1)));
    HIPCHK(be::dmalloc((void **)&M.d_ev_idx, sizeof(long long) * std::max<size_t>(rec, 1)));
    HIPCHK(be::dmalloc((void **)&M.d_ev_ab, sizeof(double) * std::max<size_t>(rec * 2, 1)));
    HIPCHK(be::dmalloc((void **)&M.d_ev_state, sizeof(int) * std::max<size_t>(tri, 1)));
    HIPCHK(be::dmalloc((void **)&M.d_ev_prev, sizeof(double) * std::max<size_t>((size_t)PR, 1)));
    if (!lev.empty()) HIPCHK(be::copy_h2d(M.d_ev_lev, lev.data(), sizeof(double) * lev.size()));
    HIPCHK(meas_events_zero(M.d_ev_cnt, M.d_ev_idx, M.d_ev_ab, M.d_ev_state, M.d_ev_prev, (size_t)PR, C, E));
    HIPCHK(be::device_sync());
    M.ev_lev = std::move(lev);
    M.ev_C = C;
    M.ev_E = E;
    M.events = true;
    return ACME_OK;
}

int acme_batch_get_measurement_events(acme_batch *b, long long *counts, long long *idx, double *ab, long long *count) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on || !M.events) return fail(ACME_ERR_INVALID, "no measurement events are set");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const long long end = M.length ? M.start + M.length : LLONG_MAX;
    const long long cnt = (M.pos < end ? M.pos : end) - M.start;
    if (count) *count = cnt > 0 ? cnt : 0;
    const size_t tri = (size_t)b->N * M.nrows * (size_t)M.ev_C, rec = tri * 2 * (size_t)(M.ev_E + 1);     // (the device's layout is the result's)
    if (counts && tri) HIPCHK(be::copy_d2h(counts, M.d_ev_cnt, sizeof(long long) * tri * 5));
    if (idx && rec) HIPCHK(be::copy_d2h(idx, M.d_ev_idx, sizeof(long long) * rec));
    if (ab && rec) HIPCHK(be::copy_d2h(ab, M.d_ev_ab, sizeof(double) * rec * 2));
    return ACME_OK;
}

int acme_batch_clear_measurement(acme_batch *b) { return set_measurement(b, nullptr); }

int acme_batch_reset_measurement(acme_batch *b) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    if (!b->meas.on) return fail(ACME_ERR_INVALID, "no measurement is armed");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    return meas_zero(b);
}

int acme_batch_get_measurement(acme_batch *b, double *out, long long *count) {
    join_worker(b);
    if (!b || (!out && !count)) return fail(ACME_ERR_INVALID, "null argument");
    const acme_batch::Measurement &M = b->meas;
    if (!M.on) return fail(ACME_ERR_INVALID, "no measurement is armed");
    if (M.W) return fail(ACME_ERR_INVALID, "the measurement has a series of windows: use acme_batch_get_measurement_series");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    const long long end = M.length ? M.start + M.length : LLONG_MAX;
    const long long cnt = (M.pos < end ? M.pos : end) - M.start;
    const long long c = cnt > 0 ? cnt : 0;
    if (count) *count = c;
    if (!out) return ACME_OK;
    const size_t P = (size_t)b->N * M.nrows, W = (size_t)(4 + 2 * M.H);
    std::vector<double> a(W * P);
    if (!a.empty()) HIPCHK(be::copy_d2h(a.data(), M.d_acc, sizeof(double) * a.size()));
    const double inv = 1.0 / (double)c;            // (no sample measured yet: NaN and infinities)
    for (size_t p = 0; p < P; ++p) {
        double *o = out + p * W;
        o[0] = a[p] * inv;
        o[1] = std::sqrt(a[P + p] * inv);
        o[2] = a[2 * P + p];
        o[3] = a[3 * P + p];
        for (int h = 0; h < M.H; ++h) {            // A_h = (2 / count) (C_h - j S_h)
            o[4 + 2 * h] = 2.0 * a[(4 + 2 * h) * P + p] * inv;
            o[5 + 2 * h] = -2.0 * a[(5 + 2 * h) * P + p] * inv;
        }
    }
    return ACME_OK;
}

int acme_batch_set_balance(acme_batch *b, int mode) {
    join_worker(b);
    if (!b || mode < -1 || mode > 1) return fail(ACME_ERR_INVALID, "invalid argument to acme_batch_set_balance");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    b->balance = mode;
    if (mode == 0) b->bal_valid = false;
    return ACME_OK;
}

int acme_batch_get_placement(acme_batch *b, int *slot_to_instance, long long *n_slots) {
    join_worker(b);
    if (!b || (!slot_to_instance && !n_slots)) return fail(ACME_ERR_INVALID, "null argument");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    if (n_slots) *n_slots = b->N;
    if (b->bal_valid && b->d_map_bal) {
        const long long slots = (b->N + b->bal_per - 1) / b->bal_per * BAL_SLOTS;
        if (n_slots) *n_slots = slots;
        if (slot_to_instance) HIPCHK(be::copy_d2h(slot_to_instance, b->d_map_bal, sizeof(int) * (size_t)slots));
    } else if (slot_to_instance)
        for (long long i = 0; i < b->N; ++i) slot_to_instance[i] = (int)i;
    return ACME_OK;
}

int acme_batch_wait(acme_batch *b) {
    if (!b) return fail(ACME_ERR_INVALID, "null batch");
    join_worker(b);
    if (b->slow_stream) {       // (isolation: the slow instances' launches run on a stream of the library's)
        ON_DEVICE(b);
        HIPCHK(be::stream_sync(b->slow_stream));
    }
    const int rc = b->worker_rc;
    b->worker_rc = ACME_OK;
    if (rc != ACME_OK) return fail(rc, b->worker_err);
    return ACME_OK;
}

int acme_batch_solve(acme_batch *b, int sub, const double *p, double *z, int *converged, int *iters, int mem,
                     void *stream) {
    join_worker(b);
    if (!b || !z || !converged || !iters) return fail(ACME_ERR_INVALID, "null argument to acme_batch_solve");
    if (sub < 0 || sub >= b->P.actual.nsub) return fail(ACME_ERR_INVALID, "sub-problem index out of range");
    const int np_ = b->sub_np[sub], nn_ = b->sub_nn[sub];
    if (np_ > 0 && !p) return fail(ACME_ERR_INVALID, "null p");
    if (nn_ == 0) return fail(ACME_ERR_INVALID, "model has no nonlinear sub-problem to solve");
    ON_DEVICE(b);
    be::stream_t st = (be::stream_t)stream;
    if (b->slow_stream) HIPCHK(be::stream_sync(b->slow_stream));
    const size_t pb = sizeof(double) * (size_t)b->N * (np_ ? np_ : 1), zb = sizeof(double) * (size_t)b->N * nn_,
                 ib = sizeof(int) * (size_t)b->N;
    const double *dp = p;
    double *dz = z;
    int *dc = converged, *di = iters;
    if (mem == ACME_MEM_HOST) {
        const size_t need = pb + zb + 2 * ib + 64;
        if (need > b->cap_u) {
            (void)be::dfree(b->d_u); b->d_u = nullptr; b->cap_u = 0;
            HIPCHK(be::dmalloc((void **)&b->d_u, need));
            b->cap_u = need;
        }
        char *base = (char *)b->d_u;
        if (np_) HIPCHK(be::copy_h2d_async(base, p, sizeof(double) * (size_t)b->N * np_, st));
        dp = (const double *)base;
        dz = (double *)(base + pb);
        dc = (int *)(base + pb + zb);
        di = (int *)(base + pb + zb + ib);
    } else if (mem != ACME_MEM_DEVICE) {
        return fail(ACME_ERR_INVALID, "mem must be ACME_MEM_HOST or ACME_MEM_DEVICE");
    }
    if (b->generic) {
        GArgs A{};
        fill_gargs(b, A);
        A.mode = GEN_SOLVE;
        A.T = 1;
        A.p_in = dp;
        A.z_out = dz;
        A.conv_out = dc;
        A.iters_out = di;
        A.solve_sub = sub;
        HIPCHK(be::launch_generic(A, st));
    } else {
    KArgs A{};
    fill_args(b, A);
    A.T = 1;
    A.p_in = dp;
    A.z_out = dz;
    A.conv_out = dc;
    A.iters_out = di;
    A.np_io = np_;
    A.nn_io = nn_;
    A.solve_sub = sub;
    const unsigned grid = (unsigned)((b->N + INST_PER_BLOCK - 1) / INST_PER_BLOCK);
    if (!b->kf->launch_solve) return fail(ACME_ERR_INVALID, "model has no nonlinear sub-problem to solve");
    HIPCHK(b->kf->launch_solve(A, grid, b->lds_bytes, st));
    }
    if (mem == ACME_MEM_HOST) {
        HIPCHK(be::copy_d2h_async(z, dz, zb, st));
        HIPCHK(be::copy_d2h_async(converged, dc, ib, st));
        HIPCHK(be::copy_d2h_async(iters, di, ib, st));
        HIPCHK(be::stream_sync(st));
    }
    return ACME_OK;
}

int acme_batch_get_extrapolation_jacobian(acme_batch *b, int sub, double *jac, int mem, void *stream) {
    join_worker(b);
    if (!b || !jac) return fail(ACME_ERR_INVALID, "null argument to acme_batch_get_extrapolation_jacobian");
    if (sub < 0 || sub >= b->P.actual.nsub) return fail(ACME_ERR_INVALID, "sub-problem index out of range");
    const int np_ = b->sub_np[sub], nn_ = b->sub_nn[sub];
    if (nn_ == 0 || (!b->generic && !b->kf->launch_jac)) return fail(ACME_ERR_INVALID, "model has no nonlinear sub-problem");
    if (np_ == 0) return ACME_OK;      // nn x 0 matrices: nothing to write
    ON_DEVICE(b);
    be::stream_t st = (be::stream_t)stream;
    if (b->slow_stream) HIPCHK(be::stream_sync(b->slow_stream));
    const size_t jb = sizeof(double) * (size_t)b->N * np_ * nn_;
    double *dj = jac;
    if (mem == ACME_MEM_HOST) {
        if (jb > b->cap_y) {
            (void)be::dfree(b->d_y); b->d_y = nullptr; b->cap_y = 0;
            HIPCHK(be::dmalloc((void **)&b->d_y, jb));
            b->cap_y = jb;
        }
        dj = b->d_y;
    } else if (mem != ACME_MEM_DEVICE) {
        return fail(ACME_ERR_INVALID, "mem must be ACME_MEM_HOST or ACME_MEM_DEVICE");
    }
    if (b->generic) {
        GArgs A{};
        fill_gargs(b, A);
        A.mode = GEN_JAC;
        A.jac_out = dj;
        A.solve_sub = sub;
        HIPCHK(be::launch_generic(A, st));
    } else {
    KArgs A{};
    fill_args(b, A);
    A.T = 0;
    A.jac_out = dj;
    A.np_io = np_;
    A.nn_io = nn_;
    A.solve_sub = sub;
    const unsigned grid = (unsigned)((b->N + INST_PER_BLOCK - 1) / INST_PER_BLOCK);
    HIPCHK(b->kf->launch_jac(A, grid, b->lds_bytes, st));
    }
    if (mem == ACME_MEM_HOST) {
        HIPCHK(be::copy_d2h_async(jac, dj, jb, st));
        HIPCHK(be::stream_sync(st));
    }
    return ACME_OK;
}

int acme_batch_last_kernel_ms(acme_batch *b, float *ms) {
    join_worker(b);
    if (!b || !ms) return fail(ACME_ERR_INVALID, "null argument");
    ON_DEVICE(b);
    int rc = drain_events(b, b->ev_pending);
    if (rc != ACME_OK) return rc;
    if (!b->launches) return fail(ACME_ERR_INVALID, "no kernel has been launched yet");
    *ms = b->ms_last;
    return ACME_OK;
}

int acme_batch_kernel_time(acme_batch *b, double *ms_total, long long *launches, int reset) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null argument");
    ON_DEVICE(b);
    int rc = drain_events(b, b->ev_pending);
    if (rc != ACME_OK) return rc;
    if (ms_total) *ms_total = b->ms_sum;
    if (launches) *launches = b->launches;
    if (reset) { b->ms_sum = 0.0; b->launches = 0; }
    return ACME_OK;
}

int acme_batch_get_report(acme_batch *b, acme_report *reports) {
    join_worker(b);
    if (!b || !reports) return fail(ACME_ERR_INVALID, "null argument");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    std::vector<long long> w((size_t)b->N * RW_WORDS);
    HIPCHK(be::copy_d2h(w.data(), b->d_report, w.size() * sizeof(long long)));
    for (long long i = 0; i < b->N; ++i) {
        const long long *r = &w[(size_t)i * RW_WORDS];
        reports[i].n_warn = r[RW_NWARN];
        reports[i].first_nonconverged = r[RW_FIRST_NONCONV];
        reports[i].first_nonfinite = r[RW_FIRST_NONFINITE];
        reports[i].iters_total = r[RW_ITERS_TOTAL];
        reports[i].iters_max = r[RW_ITERS_MAX];
    }
    return ACME_OK;
}

int acme_batch_reset_report(acme_batch *b) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null argument");
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    std::vector<long long> w((size_t)b->N * RW_WORDS, 0);
    for (long long i = 0; i < b->N; ++i) {
        w[(size_t)i * RW_WORDS + RW_FIRST_NONCONV] = -1;
        w[(size_t)i * RW_WORDS + RW_FIRST_NONFINITE] = -1;
    }
    HIPCHK(be::copy_h2d(b->d_report, w.data(), w.size() * sizeof(long long)));
    b->samples_done = 0;
    // (the counters the isolation and the placement of the waves difference start over; groups and placement stay)
    b->iso_samples = 0;
    b->iso_iters.assign(b->iso_iters.size(), 0);
    b->bal_samples = 0;
    if (b->d_bal_prev) {
        std::vector<long long> z((size_t)b->N, 0);
        HIPCHK(be::copy_h2d(b->d_bal_prev, z.data(), sizeof(long long) * z.size()));
    }
    return ACME_OK;
}

int acme_batch_set_resabstol(acme_batch *b, double tol) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null argument");
    b->o.tol = tol;
    return ACME_OK;
}

// x is [N][nx]; p is [N][sum of np_k]; z is [N][sum of nn_k] (sub-problems concatenated in order)
static int state_io(acme_batch *b, double *x, double *p, double *z, const double *cx, const double *cp,
                    const double *cz, bool set) {
    ON_DEVICE(b);
    HIPCHK(be::device_sync());
    if (b->generic) {       // x | last_p of every sub-problem | last_z of every sub-problem: the caller's own layout
        const GenHeader &H = b->G.H;
        const int S = H.state_total;
        std::vector<double> st((size_t)b->N * (S ? S : 1));
        if (S) HIPCHK(be::copy_d2h(st.data(), b->d_state, sizeof(double) * (size_t)b->N * S));
        for (long long i = 0; i < b->N; ++i) {
            double *r = &st[(size_t)i * S];
            for (int k = 0; k < H.nx; ++k) { if (set) { if (cx) r[k] = cx[i * H.nx + k]; } else if (x) x[i * H.nx + k] = r[k]; }
            for (int k = 0; k < H.npt; ++k) { if (set) { if (cp) r[H.nx + k] = cp[i * H.npt + k]; } else if (p) p[i * H.npt + k] = r[H.nx + k]; }
            for (int k = 0; k < H.nnt; ++k) { if (set) { if (cz) r[H.nx + H.npt + k] = cz[i * H.nnt + k]; } else if (z) z[i * H.nnt + k] = r[H.nx + H.npt + k]; }
        }
        if (set && S) HIPCHK(be::copy_h2d(b->d_state, st.data(), sizeof(double) * (size_t)b->N * S));
        return ACME_OK;
    }
    const int S = b->k->state;
    const Dims &s = b->P.shape, &a = b->P.actual;
    const int nsubr = s.nsub > 0 ? s.nsub : 1;
    int npt = 0, nnt = 0;
    for (int k = 0; k < a.nsub; ++k) { npt += b->sub_np[k]; nnt += b->sub_nn[k]; }
    std::vector<double> st((size_t)b->N * (S ? S : 1));
    if (S) HIPCHK(be::copy_d2h(st.data(), b->d_state, sizeof(double) * (size_t)b->N * S));
    for (long long i = 0; i < b->N; ++i) {
        double *r = &st[(size_t)i * S];
        if (set) { if (cx) for (int k = 0; k < a.nx; ++k) r[k] = cx[i * a.nx + k]; }
        else     { if (x)  for (int k = 0; k < a.nx; ++k) x[i * a.nx + k] = r[k]; }
        int po = 0, zo = 0;
        for (int sub = 0; sub < a.nsub; ++sub) {
            double *rp = r + s.nx + sub * s.np, *rz = r + s.nx + nsubr * s.np + sub * s.nn;
            for (int k = 0; k < b->sub_np[sub]; ++k) {
                if (set) { if (cp) rp[k] = cp[i * npt + po + k]; }
                else if (p) p[i * npt + po + k] = rp[k];
            }
            for (int k = 0; k < b->sub_nn[sub]; ++k) {      // (condensed shapes: the kernel's z basis is permuted)
                const int kk = s.nl > 0 ? b->P.zinv[k] : k;
                if (set) { if (cz) rz[kk] = cz[i * nnt + zo + k]; }
                else if (z) z[i * nnt + zo + k] = rz[kk];
            }
            po += b->sub_np[sub];
            zo += b->sub_nn[sub];
        }
    }
    if (set && S) HIPCHK(be::copy_h2d(b->d_state, st.data(), sizeof(double) * (size_t)b->N * S));
    if (set && (cp || cz)) {     // an origin set from outside need not satisfy the linear rows
        std::vector<int> cf((size_t)b->N, 1);
        HIPCHK(be::copy_h2d(b->d_cflags, cf.data(), sizeof(int) * cf.size()));
    }
    return ACME_OK;
}

int acme_batch_get_state(acme_batch *b, double *x, double *p, double *z) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null argument");
    return state_io(b, x, p, z, nullptr, nullptr, nullptr, false);
}

int acme_batch_set_state(acme_batch *b, const double *x, const double *p, const double *z) {
    join_worker(b);
    if (!b) return fail(ACME_ERR_INVALID, "null argument");
    return state_io(b, nullptr, nullptr, nullptr, x, p, z, true);
}

}  // extern "C"
