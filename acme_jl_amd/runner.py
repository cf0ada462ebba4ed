"""ModelRunner / run: the host-side mirror of the reference's runner API over the C ABI.

Reference interface mirrored (src/ACME.jl):
  * ``ModelRunner(model, showprogress)`` ............ :570-604
  * ``run!(runner, u)`` / ``run!(runner, y, u)`` ..... :619-664 (+ ``checkiosizes`` :625-635)
  * ``run!(model, u)`` ............................... :567-568
  * failure policy of ``step!`` ....................... :688-694
  * ``set_resabstol!`` / extrapolation origin ......... src/solvers.jl:181-198

The difference to the reference is the batch axis: one runner advances ``n_instances``
independent copies of the circuit in lock step on one GPU.  All compute happens in
``libacme_hip.so`` (hand-written HIP for gfx950).  There is NO CPU fallback: if the
library or a GPU is missing, constructing a runner raises.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings

import numpy as np

from .model import SOLVER_IDS, CachingHomotopySolver, DiscreteModel

_HERE = os.path.dirname(os.path.abspath(__file__))
# ACME_HIP_LIB: developer override used to A/B kernel build variants (tools/variants.sh)
DEFAULT_LIBRARY = os.environ.get("ACME_HIP_LIB") or os.path.join(_HERE, "csrc", "libacme_hip.so")

ACME_MEM_HOST, ACME_MEM_DEVICE = 0, 1


class DimensionMismatch(ValueError):
    """Julia's DimensionMismatch (src/ACME.jl:625-635)."""


class AcmeError(RuntimeError):
    pass


class Options(C.Structure):
    _fields_ = [("solver", C.c_int), ("tol", C.c_double), ("maxiter", C.c_int),
                ("device", C.c_int), ("per_instance_matrices", C.c_int)]


class Report(C.Structure):
    _fields_ = [("n_warn", C.c_longlong), ("first_nonconverged", C.c_longlong),
                ("first_nonfinite", C.c_longlong), ("iters_total", C.c_longlong),
                ("iters_max", C.c_longlong)]


# every symbol include/acme_hip.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "acme_last_error", "acme_device_count", "acme_default_options", "acme_model_create",
    "acme_model_add_subproblem", "acme_model_set_row_order", "acme_model_destroy",
    "acme_model_kernel_shape", "acme_model_kernel_variant",
    "acme_batch_create", "acme_batch_destroy", "acme_batch_kernel_variant", "acme_batch_set_matrices", "acme_batch_run", "acme_batch_run_const",
    "acme_batch_run_async", "acme_batch_wait", "acme_batch_set_host_retention", "acme_batch_release_host_buffers", "acme_batch_set_progress_callback", "acme_batch_set_isolation",
    "acme_batch_set_balance", "acme_batch_get_placement",
    "acme_batch_solve", "acme_batch_get_extrapolation_jacobian", "acme_batch_last_kernel_ms", "acme_batch_kernel_time", "acme_batch_get_report", "acme_batch_reset_report",
    "acme_batch_set_resabstol", "acme_batch_get_state", "acme_batch_set_state",
    "acme_oversampling_design", "acme_batch_set_oversampling",
    "acme_batch_set_measurement", "acme_batch_clear_measurement", "acme_batch_reset_measurement", "acme_batch_get_measurement",
    "acme_batch_set_measurement_per_instance", "acme_batch_get_measurement_plan",
    "acme_batch_set_source_const", "acme_batch_set_source_sine", "acme_batch_set_source_table", "acme_batch_clear_source",
    "acme_batch_set_source_clock", "acme_batch_get_source_clock", "acme_batch_run_sources", "acme_batch_run_sources_async",
    "acme_batch_render_sources",
    "acme_batch_set_source_multisine", "acme_batch_set_source_noise", "acme_batch_set_source_pulse", "acme_batch_set_source_burst",
    "acme_batch_set_measurement_bins",
    "acme_batch_set_measurement_series", "acme_batch_get_measurement_series",
    "acme_batch_set_measurement_fold", "acme_batch_get_measurement_fold", "acme_batch_get_measurement_fold_sums",
    "acme_batch_set_measurement_spectrum", "acme_batch_get_measurement_spectrum", "acme_batch_get_measurement_spectrum_sums",
    "acme_batch_get_measurement_spectrum_table",
    "acme_batch_set_measurement_cross", "acme_batch_get_measurement_cross", "acme_batch_get_measurement_cross_sums",
    "acme_batch_get_measurement_cross_table",
    "acme_batch_set_measurement_target", "acme_batch_get_measurement_target",
    "acme_batch_set_measurement_weighting", "acme_batch_get_measurement_weighting",
    "acme_batch_set_measurement_ensemble", "acme_batch_get_measurement_ensemble",
    "acme_batch_set_measurement_histogram", "acme_batch_get_measurement_histogram",
    "acme_batch_set_measurement_events", "acme_batch_get_measurement_events",
]

SOURCE_CONST, SOURCE_SINE, SOURCE_TABLE, SOURCE_MULTISINE, SOURCE_NOISE, SOURCE_PULSE, SOURCE_BURST = 1, 2, 3, 4, 5, 6, 7
MAX_PULSE_PERIOD = 2 ** 31 - 1
NOISE_UNIFORM, NOISE_GAUSSIAN = 0, 1
MAX_SOURCE_TONES = 4
MAX_FOLD_PERIOD = 65536
MAX_TARGETS = 64
MAX_WEIGHTING_SECTIONS = 8
MAX_ENSEMBLE = 16777216
HIST_SIGNED, HIST_ABS = 0, 1
MAX_HIST_BINS = 4096
MAX_HISTOGRAM = 268435456
MAX_EVENT_LEVELS, MAX_EVENT_SLOTS = 8, 16
MAX_EVENTS = 16777216
EVENT_RISE, EVENT_FALL, EVENT_HIGH, EVENT_LOW, EVENT_UNKNOWN = 0, 1, 2, 3, 4
_SOURCE_KINDS = {"const": SOURCE_CONST, "sine": SOURCE_SINE, "table": SOURCE_TABLE, "multisine": SOURCE_MULTISINE, "noise": SOURCE_NOISE,
                 SOURCE_CONST: SOURCE_CONST, SOURCE_SINE: SOURCE_SINE, SOURCE_TABLE: SOURCE_TABLE, SOURCE_MULTISINE: SOURCE_MULTISINE,
                 SOURCE_NOISE: SOURCE_NOISE, "pulse": SOURCE_PULSE, "burst": SOURCE_BURST, "step": SOURCE_PULSE,
                 SOURCE_PULSE: SOURCE_PULSE, SOURCE_BURST: SOURCE_BURST}
_NOISE_DISTS = {"uniform": NOISE_UNIFORM, "gaussian": NOISE_GAUSSIAN, NOISE_UNIFORM: NOISE_UNIFORM, NOISE_GAUSSIAN: NOISE_GAUSSIAN}


def noise_streams(n, stream=None, seed=0):
    """The streams of a noise source over instances 0 ... n - 1 as the ABI takes them (int64; a stream is an unsigned 64-bit
    value, so 2^63 ... 2^64 - 1 wrap to the negative integers): ``stream`` -- n integers -- or ``seed * 2^32 + i``"""
    if stream is None:
        if not 0 <= int(seed) < 2 ** 31 or int(seed) != seed:
            raise ValueError("a noise source's seed must be an integer 0 ... 2^31 - 1")
        return (np.int64(int(seed)) << np.int64(32)) + np.arange(n, dtype=np.int64)
    vals = [int(v) for v in np.asarray(stream, dtype=object).ravel()]
    if len(vals) != n:
        raise DimensionMismatch(f"a noise source's streams need {n} values")
    if any(v != w for v, w in zip(vals, np.asarray(stream, dtype=object).ravel())) or not all(-2 ** 63 <= v < 2 ** 64 for v in vals):
        raise DimensionMismatch("a noise source's streams must be 64-bit integers")
    return np.array([v - 2 ** 64 if v >= 2 ** 63 else v for v in vals], dtype=np.int64)


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  If libacme_hip.so pulled in the
    system ROCm runtime first, torch would later be bound to that second, mismatching runtime
    ("No HIP GPUs are available").  Loading torch's copy first -- without importing torch --
    makes both share one HIP runtime regardless of import order.  Without torch installed
    (e.g. the Julia ccall route) the system runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            return C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            return None
    return None


# acme_progress_fn(user, samples_done, samples_total)
PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_longlong, C.c_longlong)


class Library:
    """ctypes binding of one shared library implementing include/acme_hip.h."""

    def __init__(self, path=DEFAULT_LIBRARY):
        if os.path.abspath(path) == os.path.abspath(DEFAULT_LIBRARY):
            self._hip_rt = _preload_torch_hip_runtime()
        if not os.path.exists(path):
            raise AcmeError(
                f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                " (hipcc --offload-arch=gfx950).  acme_jl_amd has no CPU fallback.")
        self.path = path
        L = self.L = C.CDLL(path)
        dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
        L.acme_last_error.restype = C.c_char_p
        L.acme_device_count.restype = C.c_int
        L.acme_default_options.argtypes = [C.POINTER(Options)]
        L.acme_model_create.argtypes = [C.c_int] * 4 + [dp] * 8 + [C.POINTER(vp)]
        L.acme_model_add_subproblem.argtypes = [vp, C.c_int, C.c_int, C.c_int] + [dp] * 7 + \
            [C.c_int, ip, ip, ip, dp]
        L.acme_model_set_row_order.argtypes = [vp, C.c_int, ip, C.c_int]
        L.acme_model_destroy.argtypes = [vp]
        L.acme_model_destroy.restype = None
        L.acme_model_kernel_shape.argtypes = [vp, ip]
        L.acme_model_kernel_variant.argtypes = [vp, ip, ip]
        L.acme_batch_create.argtypes = [vp, C.c_longlong, C.POINTER(Options), C.POINTER(vp)]
        L.acme_batch_destroy.argtypes = [vp]
        L.acme_batch_destroy.restype = None
        L.acme_batch_kernel_variant.argtypes = [vp, ip, ip]
        L.acme_batch_set_matrices.argtypes = [vp, C.c_longlong, C.c_longlong, C.POINTER(vp)]
        L.acme_batch_run.argtypes = [vp, vp, vp, C.c_longlong, C.c_int, vp]
        L.acme_batch_run_const.argtypes = [vp, vp, vp, C.c_ulonglong, vp, C.c_longlong, C.c_int, vp]
        L.acme_batch_run_async.argtypes = [vp, vp, vp, C.c_longlong, C.c_int, vp]
        L.acme_batch_wait.argtypes = [vp]
        L.acme_batch_set_host_retention.argtypes = [vp, C.c_int]
        L.acme_batch_release_host_buffers.argtypes = [vp]
        L.acme_batch_set_isolation.argtypes = [vp, C.c_double]
        L.acme_batch_set_balance.argtypes = [vp, C.c_int]
        L.acme_batch_get_placement.argtypes = [vp, ip, C.POINTER(C.c_longlong)]
        L.acme_batch_set_progress_callback.argtypes = [vp, PROGRESS_FN, vp]
        L.acme_batch_solve.argtypes = [vp, C.c_int, dp, dp, ip, ip, C.c_int, vp]
        L.acme_batch_get_extrapolation_jacobian.argtypes = [vp, C.c_int, dp, C.c_int, vp]
        L.acme_batch_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.acme_batch_kernel_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.c_int]
        L.acme_batch_get_report.argtypes = [vp, C.POINTER(Report)]
        L.acme_batch_reset_report.argtypes = [vp]
        L.acme_batch_set_resabstol.argtypes = [vp, C.c_double]
        L.acme_batch_get_state.argtypes = [vp, dp, dp, dp]
        L.acme_batch_set_state.argtypes = [vp, dp, dp, dp]
        L.acme_oversampling_design.argtypes = [C.c_int, dp, C.c_int]
        L.acme_batch_set_oversampling.argtypes = [vp, C.c_int, dp, C.c_int, dp, C.c_int, C.c_ulonglong]
        L.acme_batch_set_measurement.argtypes = [vp, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, C.c_ulonglong]
        L.acme_batch_set_measurement_per_instance.argtypes = [vp, C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong),
                                                              C.c_int, C.c_ulonglong]
        L.acme_batch_get_measurement_plan.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                                      C.POINTER(C.c_int)]
        L.acme_batch_clear_measurement.argtypes = [vp]
        L.acme_batch_reset_measurement.argtypes = [vp]
        L.acme_batch_get_measurement.argtypes = [vp, dp, C.POINTER(C.c_longlong)]
        lp = C.POINTER(C.c_longlong)
        L.acme_batch_set_source_const.argtypes = [vp, C.c_int, dp]
        L.acme_batch_set_source_sine.argtypes = [vp, C.c_int, C.c_longlong, lp, lp, dp, dp]
        L.acme_batch_set_source_table.argtypes = [vp, C.c_int, dp, C.c_longlong, dp, dp]
        L.acme_batch_clear_source.argtypes = [vp, C.c_int]
        L.acme_batch_set_source_clock.argtypes = [vp, C.c_longlong]
        L.acme_batch_get_source_clock.argtypes = [vp, lp]
        L.acme_batch_run_sources.argtypes = [vp, vp, vp, C.c_longlong, C.c_int, vp]
        L.acme_batch_run_sources_async.argtypes = [vp, vp, vp, C.c_longlong, C.c_int, vp]
        L.acme_batch_render_sources.argtypes = [vp, vp, vp, C.c_longlong, C.c_int, vp]
        L.acme_batch_set_source_multisine.argtypes = [vp, C.c_int, C.c_longlong, C.c_int, lp, lp, dp, dp]
        L.acme_batch_set_source_noise.argtypes = [vp, C.c_int, C.c_int, C.c_longlong, lp, dp, dp]
        L.acme_batch_set_source_pulse.argtypes = [vp, C.c_int, lp, dp, dp]
        L.acme_batch_set_source_burst.argtypes = [vp, C.c_int, lp, C.c_longlong, lp, lp, dp, dp]
        L.acme_batch_set_measurement_bins.argtypes = [vp, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, lp, C.c_int, ip,
                                                      C.c_ulonglong]
        L.acme_batch_set_measurement_series.argtypes = [vp, C.c_longlong, C.c_longlong, C.c_longlong]
        L.acme_batch_get_measurement_series.argtypes = [vp, C.c_longlong, C.c_longlong, dp, lp]
        L.acme_batch_set_measurement_fold.argtypes = [vp, C.c_longlong, lp]
        L.acme_batch_get_measurement_fold.argtypes = [vp, dp, lp, lp]
        L.acme_batch_get_measurement_fold_sums.argtypes = [vp, dp]
        L.acme_batch_set_measurement_spectrum.argtypes = [vp, C.c_longlong, C.c_longlong, dp]
        L.acme_batch_get_measurement_spectrum.argtypes = [vp, dp, lp, lp]
        L.acme_batch_get_measurement_spectrum_sums.argtypes = [vp, dp]
        L.acme_batch_get_measurement_spectrum_table.argtypes = [vp, dp, dp]
        L.acme_batch_set_measurement_cross.argtypes = [vp, C.c_int, C.c_longlong, C.c_longlong, dp]
        L.acme_batch_get_measurement_cross.argtypes = [vp, dp, lp, lp]
        L.acme_batch_get_measurement_cross_sums.argtypes = [vp, dp]
        L.acme_batch_get_measurement_cross_table.argtypes = [vp, dp, dp]
        L.acme_batch_set_measurement_target.argtypes = [vp, dp, C.c_longlong, C.c_longlong, ip, lp, C.c_double]
        L.acme_batch_get_measurement_target.argtypes = [vp, dp, lp]
        L.acme_batch_set_measurement_ensemble.argtypes = [vp, ip, C.c_int, C.c_longlong]
        L.acme_batch_get_measurement_ensemble.argtypes = [vp, dp, lp, lp, lp]
        L.acme_batch_set_measurement_histogram.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, dp, dp]
        L.acme_batch_get_measurement_histogram.argtypes = [vp, lp, dp, lp]
        L.acme_batch_set_measurement_events.argtypes = [vp, C.c_int, dp, dp, C.c_int]
        L.acme_batch_get_measurement_events.argtypes = [vp, lp, lp, dp, lp]
        L.acme_batch_set_measurement_weighting.argtypes = [vp, dp, C.c_int]
        L.acme_batch_get_measurement_weighting.argtypes = [vp, dp, C.POINTER(C.c_int)]

    def check(self, rc):
        if rc < 0:
            raise AcmeError(self.L.acme_last_error().decode())
        return rc

    def device_count(self):
        return self.L.acme_device_count()


_DEFAULT = None


def default_library():
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Library(DEFAULT_LIBRARY)
    return _DEFAULT


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def design_oversampling_filter(factor, lib=None):
    """The library's default lowpass for oversampling by ``factor`` (``acme_oversampling_design``): a linear-phase
    Kaiser-windowed sinc at the high rate, unit DC gain, passband to 0.40 fs, at least 80 dB from 0.50 fs, length
    L = 1 (mod factor) and odd.  The one design ``set_oversampling`` uses when no taps are given."""
    lib = lib or default_library()
    n = lib.check(lib.L.acme_oversampling_design(int(factor), None, 0))
    taps = np.zeros(n)
    lib.check(lib.L.acme_oversampling_design(int(factor), _dp(taps), n))
    return taps


class Measurement:
    """What ``ModelRunner.measurement()`` returns: per instance and measured output row (``rows``, ascending) the window's
    ``mean``, ``rms``, ``min``, ``max`` and ``peak`` (N, nrows), and ``harmonics`` (N, nrows, H), the complex amplitudes
    A_h = (2 / count) sum_m y[m] exp(-j h w m) of the fundamental's harmonics h = 1 ... H; ``count`` samples were measured.
    After ``set_measurement_bins`` the same array is the bins' complex amplitudes A_b (N, nrows, B), also as ``bins``."""

    def __init__(self, out, count, rows):
        self.count = int(count)
        self.rows = tuple(rows)
        self.mean, self.rms, self.min, self.max = (out[:, :, k].copy() for k in range(4))
        self.harmonics = out[:, :, 4::2] + 1j * out[:, :, 5::2]

    @property
    def bins(self):
        """the complex amplitudes of a bins measurement (N, nrows, B), in the order of ``coef``"""
        return self.harmonics

    def imd(self, fundamental_bins, product_bins):
        """intermodulation distortion (N, nrows): the root-sum-square of the amplitudes of the bins ``product_bins`` over
        that of the bins ``fundamental_bins`` (indices into ``bins``)"""
        a = np.abs(self.harmonics)
        fb, pb = list(fundamental_bins), list(product_bins)
        if not fb or not pb:
            raise ValueError("IMD needs at least one fundamental bin and one product bin")
        return np.sqrt((a[:, :, pb] ** 2).sum(axis=2)) / np.sqrt((a[:, :, fb] ** 2).sum(axis=2))

    @property
    def peak(self):
        return np.maximum(np.abs(self.min), np.abs(self.max))

    def loudness(self):
        """the window's loudness ``-0.691 + 10 log10(sum y^2 / count)`` (N, nrows), LKFS when the measurement carries the K
        weighting (``weighting_sos("K", fs)``) and the window is a 400 ms block of BS.1770"""
        with np.errstate(divide="ignore"):
            return -0.691 + 10.0 * np.log10(self.rms * self.rms)

    def thd(self):
        """total harmonic distortion sqrt(sum_{h >= 2} |A_h|^2) / |A_1| (N, nrows); needs H >= 2"""
        a = np.abs(self.harmonics)
        if a.shape[2] < 2:
            raise ValueError("THD needs a measurement of at least 2 harmonics")
        return np.sqrt((a[:, :, 1:] ** 2).sum(axis=2)) / a[:, :, 0]

    @classmethod
    def concatenate(cls, parts):
        m = cls.__new__(cls)
        m.count, m.rows = parts[0].count, parts[0].rows
        for k in ("mean", "rms", "min", "max", "harmonics"):
            setattr(m, k, np.concatenate([getattr(p, k) for p in parts]))
        return m


class MeasurementSeries:
    """What ``ModelRunner.measurement_series()`` returns: the windows ``first ... first + len() - 1`` of a series.  Indexing
    yields a window's ``Measurement``; ``counts`` (W,) the samples measured so far per window, ``complete`` the number of
    windows with ``count == win``, ``starts`` (W,) each window's first sample counted from arming; ``mean``, ``rms``, ``min``,
    ``max``, ``peak`` stacked (W, N, nrows), ``harmonics`` / ``bins`` (W, N, nrows, H); ``thd()`` / ``imd()`` (W, N, nrows)."""

    def __init__(self, out, counts, rows, start, win, hop, first=0):
        self.counts = np.asarray(counts, dtype=np.int64)
        self.rows = tuple(rows)
        self.win, self.hop, self.first = int(win), int(hop), int(first)
        self.starts = int(start) + (self.first + np.arange(len(self.counts), dtype=np.int64)) * self.hop
        self.mean, self.rms, self.min, self.max = (out[..., k].copy() for k in range(4))
        self.harmonics = out[..., 4::2] + 1j * out[..., 5::2]

    def __len__(self):
        return len(self.counts)

    def __getitem__(self, w):
        w = range(len(self))[w]         # (negative indices, IndexError beyond the series)
        m = Measurement.__new__(Measurement)
        m.count, m.rows = int(self.counts[w]), self.rows
        for k in ("mean", "rms", "min", "max", "harmonics"):
            setattr(m, k, getattr(self, k)[w])
        return m

    @property
    def complete(self):
        return int((self.counts == self.win).sum())

    @property
    def bins(self):
        return self.harmonics

    @property
    def peak(self):
        return np.maximum(np.abs(self.min), np.abs(self.max))

    def loudness(self, blocks=1):
        """the loudness ``-0.691 + 10 log10(sum y^2 / count)`` per window (W, N, nrows), as ``Measurement.loudness``.
        ``blocks`` > 1: of every run of ``blocks`` consecutive windows taken together (W - blocks + 1, N, nrows), for a series
        of back-to-back windows (``hop == win``; a series does not take overlapping windows) -- behind the K weighting,
        windows of 100 ms with ``blocks=4`` are the 400 ms blocks every 100 ms of BS.1770.  Complete windows only."""
        ms = self.rms * self.rms
        if blocks > 1:
            if self.hop != self.win:
                raise ValueError("loudness over several windows needs a series of back-to-back windows (hop == win)")
            n = len(ms) - blocks + 1
            ms = sum(ms[k:k + max(n, 0)] for k in range(blocks)) / blocks
        with np.errstate(divide="ignore"):
            return -0.691 + 10.0 * np.log10(ms)

    def thd(self):
        """total harmonic distortion per window (W, N, nrows); needs H >= 2"""
        a = np.abs(self.harmonics)
        if a.shape[-1] < 2:
            raise ValueError("THD needs a measurement of at least 2 harmonics")
        return np.sqrt((a[..., 1:] ** 2).sum(axis=-1)) / a[..., 0]

    def imd(self, fundamental_bins, product_bins):
        """intermodulation distortion per window (W, N, nrows), as ``Measurement.imd``"""
        a = np.abs(self.harmonics)
        fb, pb = list(fundamental_bins), list(product_bins)
        if not fb or not pb:
            raise ValueError("IMD needs at least one fundamental bin and one product bin")
        return np.sqrt((a[..., pb] ** 2).sum(axis=-1)) / np.sqrt((a[..., fb] ** 2).sum(axis=-1))

    @classmethod
    def concatenate(cls, parts):
        m = cls.__new__(cls)
        for k in ("counts", "rows", "win", "hop", "first", "starts"):
            setattr(m, k, getattr(parts[0], k))
        for k in ("mean", "rms", "min", "max", "harmonics"):
            setattr(m, k, np.concatenate([getattr(p, k) for p in parts], axis=1))
        return m


class MeasurementFold:
    """What ``ModelRunner.measurement_fold()`` returns: the measured window folded onto one period per instance
    (synchronous averaging).  ``mean`` (N, nrows, Pmax): slot s of instance i, s < ``period[i]``, holds the mean of the
    window's samples m with m mod period[i] == s; slots no sample has reached, and the slots at and beyond an instance's
    period, are NaN.  ``period`` (N,), ``count`` the samples measured, ``rows`` the measured output rows."""

    def __init__(self, mean, period, count, rows):
        self.mean, self.period, self.count, self.rows = mean, np.asarray(period, dtype=np.int64), int(count), tuple(rows)

    def slot_counts(self, i):
        """the samples each slot of instance ``i`` has received (period[i],)"""
        P = int(self.period[i])
        s = np.arange(P)
        return np.where(self.count > s, (self.count - s - 1) // P + 1, 0)

    def spectrum(self, i, row=0):
        """the complex amplitudes of the lines k / period[i] of the sample rate, k = 0 ... period[i] // 2, of instance
        ``i``'s folded period (``row``: index into ``rows``): ``2 / P rfft(mean[i, row, :P])`` -- the scaling of a
        measurement's A_h, line k the harmonic A_k of the fundamental 1 / P --, the DC line (the mean) unscaled"""
        P = int(self.period[i])
        a = np.fft.rfft(self.mean[i, row, :P]) * (2.0 / P)
        a[0] *= 0.5
        return a

    @classmethod
    def concatenate(cls, parts):
        if any((p.count, p.rows) != (parts[0].count, parts[0].rows) for p in parts):
            raise ValueError("the shards' folds differ in their sample counts or measured rows")
        pm = max(p.mean.shape[2] for p in parts)
        mean = np.concatenate([np.pad(p.mean, ((0, 0), (0, 0), (0, pm - p.mean.shape[2])), constant_values=np.nan) for p in parts])
        return cls(mean, np.concatenate([p.period for p in parts]), parts[0].count, parts[0].rows)


class MeasurementSpectrum:
    """What ``ModelRunner.measurement_spectrum()`` returns: Welch-averaged periodograms of the measured window.  ``power``
    (N, nrows, nfft / 2 + 1): the mean over ``segments`` segments of |FFT(w x)|^2, unscaled (NaN while ``segments`` is 0;
    ``raw``: the sums); ``count`` the samples measured, ``rows`` the measured output rows, ``window`` the nfft window
    values, ``hop`` the segments' spacing."""

    def __init__(self, power, segments, count, rows, window, hop):
        self.power, self.segments, self.count, self.rows = power, int(segments), int(count), tuple(rows)
        self.window, self.hop = np.asarray(window, dtype=np.float64), int(hop)

    @property
    def nfft(self):
        return len(self.window)

    def freqs(self, fs):
        """the bins' frequencies, k fs / nfft"""
        return np.arange(self.nfft // 2 + 1) * (float(fs) / self.nfft)

    def psd(self, fs):
        """the one-sided power spectral density, ``power / (fs sum w^2)``, doubled except at DC and Nyquist (what
        ``scipy.signal.welch(..., scaling="density", detrend=False)`` reports)"""
        d = self.power / (float(fs) * np.sum(self.window ** 2))
        d[..., 1:-1] *= 2.0
        return d

    def band_power(self, fs, f_lo, f_hi):
        """the power in f_lo <= f <= f_hi: the density's bins there times the bin width fs / nfft -- (N, nrows)"""
        f = self.freqs(fs)
        return self.psd(fs)[..., (f >= f_lo) & (f <= f_hi)].sum(axis=-1) * (float(fs) / self.nfft)

    def amplitude(self):
        """the amplitude of a line that sits on a bin, ``2 sqrt(power) / sum w`` (DC and Nyquist read twice their value)"""
        return 2.0 * np.sqrt(self.power) / np.sum(self.window)

    @classmethod
    def concatenate(cls, parts):
        a = parts[0]
        if any((p.segments, p.count, p.rows, p.hop) != (a.segments, a.count, a.rows, a.hop) or not np.array_equal(p.window, a.window)
               for p in parts):
            raise ValueError("the shards' spectra differ in their segments, sample counts, measured rows or windows")
        return cls(np.concatenate([p.power for p in parts]), a.segments, a.count, a.rows, a.window, a.hop)


class MeasurementCross:
    """What ``ModelRunner.measurement_cross()`` returns: the Welch-averaged auto- and cross-spectra of input row ``in_row``
    (x) and the measured output rows (y).  ``sxx``, ``syy`` (N, nrows, nfft / 2 + 1) real and ``sxy`` complex: the means over
    ``segments`` segments of |X|^2, |Y|^2 and conj(X) Y with X, Y = FFT(w x), FFT(w y), unscaled (NaN while ``segments`` is 0;
    ``raw``: the sums); ``count`` the samples measured, ``rows`` the measured output rows, ``window`` the nfft window
    values, ``hop`` the segments' spacing."""

    def __init__(self, sxx, syy, sxy, segments, count, rows, in_row, window, hop):
        self.sxx, self.syy, self.sxy = sxx, syy, sxy
        self.segments, self.count, self.rows, self.in_row = int(segments), int(count), tuple(rows), int(in_row)
        self.window, self.hop = np.asarray(window, dtype=np.float64), int(hop)

    @property
    def nfft(self):
        return len(self.window)

    def freqs(self, fs):
        """the bins' frequencies, k fs / nfft"""
        return np.arange(self.nfft // 2 + 1) * (float(fs) / self.nfft)

    def transfer(self, estimator="h1"):
        """the frequency response from x to y: "h1", ``sxy / sxx`` (unbiased under noise on the output), or "h2",
        ``syy / conj(sxy)`` (under noise on the input) -- complex (N, nrows, nfft / 2 + 1)"""
        if estimator == "h1":
            return self.sxy / self.sxx
        if estimator == "h2":
            return self.syy / np.conj(self.sxy)
        raise ValueError(f"estimator {estimator!r}: \"h1\" or \"h2\"")

    def coherence(self):
        """the magnitude-squared coherence ``|sxy|^2 / (sxx syy)``: 1 where y depends linearly on x alone"""
        return (self.sxy.real ** 2 + self.sxy.imag ** 2) / (self.sxx * self.syy)

    def _psd(self, power, fs):
        d = power / (float(fs) * np.sum(self.window ** 2))
        d[..., 1:-1] *= 2.0
        return d

    def input_psd(self, fs):
        """the one-sided power spectral density of x, scaled as ``MeasurementSpectrum.psd``"""
        return self._psd(self.sxx, fs)

    def output_psd(self, fs):
        """the one-sided power spectral density of y, scaled as ``MeasurementSpectrum.psd``"""
        return self._psd(self.syy, fs)

    @classmethod
    def concatenate(cls, parts):
        a = parts[0]
        if any((p.segments, p.count, p.rows, p.in_row, p.hop) != (a.segments, a.count, a.rows, a.in_row, a.hop)
               or not np.array_equal(p.window, a.window) for p in parts):
            raise ValueError("the shards' cross-spectra differ in their segments, sample counts, rows or windows")
        return cls(*(np.concatenate([getattr(p, n) for p in parts]) for n in ("sxx", "syy", "sxy")), a.segments, a.count, a.rows,
                   a.in_row, a.window, a.hop)


class MeasurementTarget:
    """What ``ModelRunner.measurement_target()`` returns: the residual of the measured window against the target waveform,
    per instance and measured row.  ``sums`` (N, nrows, 7): the chains themselves in the order ``See, Stt, Syt, St, emax,
    Pee, Ptt`` (also as ``see`` ... ``ptt``, (N, nrows) each); ``count`` the samples measured, ``rows`` the measured output
    rows, ``y_mean`` (N, nrows) the base measurement's mean (None when read with ``raw=True``)."""
    NAMES = ("see", "stt", "syt", "st", "emax", "pee", "ptt")

    def __init__(self, sums, count, rows, y_mean=None):
        self.sums, self.count, self.rows, self.y_mean = sums, int(count), tuple(rows), y_mean
        for k, name in enumerate(self.NAMES):
            setattr(self, name, sums[:, :, k])

    @property
    def esr(self):
        """the error-to-signal ratio ``See / Stt`` = sum (y - t)^2 / sum t^2"""
        return self.see / self.stt

    @property
    def esr_preemphasis(self):
        """the error-to-signal ratio behind the pre-emphasis filter 1 - c z^-1, ``Pee / Ptt``"""
        return self.pee / self.ptt

    @property
    def gain(self):
        """the least-squares gain g of y = g t, ``Syt / Stt``"""
        return self.syt / self.stt

    @property
    def error_rms(self):
        return np.sqrt(self.see / self.count)

    @property
    def error_peak(self):
        return self.emax

    @property
    def error_mean(self):
        """the mean of y - t: the base measurement's mean of y less ``St / count``"""
        if self.y_mean is None:
            raise ValueError("error_mean needs the base measurement's mean: read measurement_target() without raw=True")
        return self.y_mean - self.st / self.count

    @property
    def null_db(self):
        """the depth of the null against the target, ``10 log10(See / Stt)`` (-inf: y == t sample for sample)"""
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(self.esr)

    @classmethod
    def concatenate(cls, parts):
        a = parts[0]
        if any((p.count, p.rows) != (a.count, a.rows) for p in parts):
            raise ValueError("the shards' targets differ in their sample counts or measured rows")
        ym = None if any(p.y_mean is None for p in parts) else np.concatenate([p.y_mean for p in parts])
        return cls(np.concatenate([p.sums for p in parts]), a.count, a.rows, ym)


class MeasurementEnsemble:
    """What ``ModelRunner.measurement_ensemble()`` returns: the statistics ACROSS the instances of each group at every
    recorded sample of the window.  ``sum``, ``sumsq``, ``min``, ``max`` (G, nrows, E): the chains themselves, undivided --
    slot e is window sample ``e * stride``; ``argmin``, ``argmax`` (G, nrows, E): the instance that set the extreme (-1: no
    member); ``members`` (G,): the groups' sizes; ``filled``: the slots recorded so far (the others, and every slot of an
    empty group, read 0.0, 0.0, +inf, -inf, -1, -1); ``rows`` the measured output rows."""

    def __init__(self, sum, sumsq, min, max, argmin, argmax, members, filled, stride, rows):
        self.sum, self.sumsq, self.min, self.max, self.argmin, self.argmax = sum, sumsq, min, max, argmin, argmax
        self.members, self.filled, self.stride, self.rows = np.asarray(members, dtype=np.int64), int(filled), int(stride), tuple(rows)

    def mean(self):
        """the ensemble average ``sum / members`` (G, nrows, E); NaN for an empty group"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sum / self.members[:, None, None]

    def std(self, ddof=0):
        """the standard deviation across a group's members, from ``sumsq`` and ``sum`` (G, nrows, E); a difference that
        rounding takes below zero reads 0.0"""
        n = self.members[:, None, None].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            var = (self.sumsq - self.sum * self.sum / n) / (n - ddof)
            return np.sqrt(np.where(var < 0.0, 0.0, var))

    def band(self, sigmas=None):
        """(lower, upper), (G, nrows, E) each: the min / max envelope -- every member's waveform lies inside --, or with
        ``sigmas=k`` the band ``mean -+ k std``"""
        if sigmas is None:
            return self.min, self.max
        m, s = self.mean(), self.std()
        return m - sigmas * s, m + sigmas * s

    def trace(self, g):
        """the waveform (nrows, E) of the one member of group ``g``, as the run produced it (-0.0 reads +0.0)"""
        if self.members[g] != 1:
            raise ValueError(f"group {g} has {int(self.members[g])} members: a trace is the waveform of a one-member group")
        return self.sum[g]

    @classmethod
    def join(cls, parts, offsets):
        """the shards' results joined by group: every group's members lie in ONE shard (the others hold its start values);
        ``offsets``: the shards' first instances, added to their indices"""
        a = parts[0]
        if any((p.filled, p.stride, p.rows, p.sum.shape) != (a.filled, a.stride, a.rows, a.sum.shape) for p in parts):
            raise ValueError("the shards' ensembles differ in their slots, strides or measured rows")
        out = [np.array(getattr(a, k)) for k in ("sum", "sumsq", "min", "max", "argmin", "argmax")]
        members = np.zeros_like(a.members)
        for p, lo in zip(parts, offsets):
            has = p.members > 0
            if (members[has] > 0).any():
                raise ValueError(f"group {int(np.flatnonzero(has & (members > 0))[0])} has members in more than one shard")
            members[has] = p.members[has]
            for o, k in zip(out, ("sum", "sumsq", "min", "max")):
                o[has] = getattr(p, k)[has]
            for o, k in zip(out[4:], ("argmin", "argmax")):
                idx = getattr(p, k)[has]
                o[has] = np.where(idx >= 0, idx + lo, idx)
        return cls(*out, members, a.filled, a.stride, a.rows)


class MeasurementHistogram:
    """What ``ModelRunner.measurement_histogram()`` returns: the amplitude distribution of every (instance, measured row).
    ``counts`` (N, nrows, B) int64: bin k of instance i holds the samples with ``x`` in ``[edges(i)[k], edges(i)[k + 1])``
    (``x`` the measured value, its magnitude in the ``"abs"`` mode); ``under``, ``over``, ``nan`` (N, nrows): the samples below
    ``lo``, at or above ``hi`` and not a number; ``count``: the samples measured -- ``counts.sum(-1) + under + over + nan ==
    count`` for every pair; ``lo``, ``hi``, ``scale`` (N,): the instances' ranges and ``B / (hi - lo)`` as the library stored
    them; ``mode`` ``"signed"`` or ``"abs"``; ``rows`` the measured output rows.

    The helpers work on the samples that have a value, ``count - nan`` of them (a pair with none reads NaN), and know nothing
    finer than a bin: at a bin edge they are exact, inside a bin they take the bin's samples as spread evenly over it."""

    def __init__(self, counts, under, over, nan, count, lo, hi, scale, mode, rows):
        self.counts, self.under, self.over, self.nan = counts, under, over, nan
        self.count, self.mode, self.rows = int(count), mode, tuple(rows)
        self.lo, self.hi, self.scale = (np.asarray(a, dtype=np.float64) for a in (lo, hi, scale))

    @property
    def bins(self):
        return self.counts.shape[-1]

    def edges(self, i):
        """the B + 1 nominal bin edges of instance ``i``: ``lo + k / scale``, the last one ``hi`` itself (at an edge the
        library's two roundings decide the side a sample falls on)"""
        e = self.lo[i] + np.arange(self.bins + 1) / self.scale[i]
        e[-1] = self.hi[i]
        return e

    def _valued(self):
        n = (self.count - self.nan).astype(np.float64)
        return np.where(n > 0, n, np.nan)

    def _cumulative(self):
        """(N, nrows, B + 1): the samples below edge k"""
        return np.concatenate([self.under[..., None], self.under[..., None] + np.cumsum(self.counts, axis=-1)], axis=-1)

    def pdf(self):
        """the density per unit of ``x`` (N, nrows, B): ``counts scale / (count - nan)``; its integral over the range is the
        share of the samples inside it"""
        return self.counts * self.scale[:, None, None] / self._valued()[..., None]

    def cdf(self):
        """the share of the samples below each edge (N, nrows, B + 1): ``cdf()[..., 0]`` the share in ``under``,
        ``1 - cdf()[..., -1]`` the share in ``over``; exact"""
        return self._cumulative() / self._valued()[..., None]

    def percentile(self, q):
        """the level below which ``q`` percent of the samples lie (N, nrows), or (len(q), N, nrows) for a sequence: linear
        inside the bin that holds the rank, NaN where the answer lies in ``under`` or ``over`` (outside the range)"""
        if np.ndim(q) > 0:
            return np.stack([self.percentile(v) for v in q])
        B, cum, n = self.bins, self._cumulative().astype(np.float64), self._valued()
        target = float(q) / 100.0 * n
        with np.errstate(invalid="ignore", divide="ignore"):
            k = (cum <= target[..., None]).sum(axis=-1) - 1         # the last edge with no more than the rank below it
            inside = (k >= 0) & (k < B)
            kk = np.clip(k, 0, B - 1)
            below = np.take_along_axis(cum, kk[..., None], axis=-1)[..., 0]
            inbin = np.take_along_axis(self.counts, kk[..., None], axis=-1)[..., 0]
            x = self.lo[:, None] + (kk + (target - below) / inbin) / self.scale[:, None]
            top = (k == B) & (target == cum[..., B])                # the rank sits exactly on the last edge
            return np.where(inside, x, np.where(top, self.hi[:, None], np.nan))

    def fraction_below(self, x):
        """the share of the samples with a value below ``x`` (a scalar or N values, one per instance), (N, nrows): exact where
        ``x`` is a bin edge, interpolated linearly inside a bin; for an ``x`` outside ``[lo, hi]`` 0.0 / 1.0 where ``under`` /
        ``over`` hold nothing, NaN where they hold samples (the range did not resolve them)"""
        B, cum = self.bins, self._cumulative().astype(np.float64)
        xv = np.broadcast_to(np.asarray(x, dtype=np.float64), self.lo.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            pos = np.where(xv == self.hi, float(B), (xv - self.lo) * self.scale)     # in bins from lo
            ok = (xv >= self.lo) & (xv <= self.hi)
            k = np.clip(np.floor(np.where(ok, pos, 0.0)), 0, B).astype(np.int64)
            frac = np.where(ok, pos, 0.0) - k
            at = np.take_along_axis(cum, np.broadcast_to(k[:, None, None], cum.shape[:2] + (1,)), axis=-1)[..., 0]
            nxt = np.take_along_axis(cum, np.broadcast_to(np.minimum(k + 1, B)[:, None, None], cum.shape[:2] + (1,)), axis=-1)[..., 0]
            inside = (at + frac[:, None] * (nxt - at)) / self._valued()
            low = np.where(self.under == 0, 0.0 * self._valued(), np.nan)           # (NaN too for a pair without a valued sample)
            high = np.where(self.over == 0, 1.0 + 0.0 * self._valued(), np.nan)
            return np.where(ok[:, None], inside, np.where((xv < self.lo)[:, None], low, np.where((xv > self.hi)[:, None], high, np.nan)))

    def fraction_above(self, x):
        """the share of the samples with a value at or above ``x``: ``1 - fraction_below(x)``"""
        return 1.0 - self.fraction_below(x)

    @classmethod
    def concatenate(cls, parts):
        """several batches' results (the shards of ``MultiDeviceRunner``) as one, along the instances"""
        a = parts[0]
        if any((p.count, p.mode, p.rows, p.bins) != (a.count, a.mode, a.rows, a.bins) for p in parts):
            raise ValueError("the shards' histograms differ in their sample counts, modes, bins or measured rows")
        cat = lambda k: np.concatenate([getattr(p, k) for p in parts])
        return cls(cat("counts"), cat("under"), cat("over"), cat("nan"), a.count, cat("lo"), cat("hi"), cat("scale"), a.mode, a.rows)


class MeasurementEvents:
    """What ``ModelRunner.measurement_events()`` returns: the level crossings of every (instance, measured row, level).  The
    raw arrays are the library's: ``counts`` (N, nrows, C, 5) int64 -- RISE, FALL, then the samples after which the state is
    HIGH, LOW, UNKNOWN, the last three summing to ``count`` --, ``idx`` (N, nrows, C, 2, E + 1) int64 the window samples ``m``
    of the recorded events (direction 0: rises, 1: falls; slots 0 ... E - 1 the first E, slot E the last so far; -1: empty) and
    ``ab`` (N, nrows, C, 2, E + 1, 2) their ``v[m - 1]`` and ``v[m]`` bit for bit; ``lo``, ``hi`` (C, N) the levels; ``rows`` the
    measured output rows.  The helpers form the times on the host, in window samples from ``start``:
    ``t = (m - 1) + (thr - a) / (b - a)`` with ``thr = hi`` for a rise and ``lo`` for a fall, ``t = m`` where ``a`` is NaN."""

    def __init__(self, counts, idx, ab, count, lo, hi, rows):
        self.counts, self.idx, self.ab = counts, idx, ab
        self.count, self.rows = int(count), tuple(rows)
        self.lo, self.hi = (np.asarray(a, dtype=np.float64) for a in (lo, hi))

    levels = property(lambda self: self.counts.shape[2])
    slots = property(lambda self: self.idx.shape[-1] - 1)
    rises = property(lambda self: self.counts[..., EVENT_RISE])
    falls = property(lambda self: self.counts[..., EVENT_FALL])
    high = property(lambda self: self.counts[..., EVENT_HIGH])
    low = property(lambda self: self.counts[..., EVENT_LOW])
    unknown = property(lambda self: self.counts[..., EVENT_UNKNOWN])

    @staticmethod
    def _direction(direction):
        d = {"rise": EVENT_RISE, "fall": EVENT_FALL, EVENT_RISE: EVENT_RISE, EVENT_FALL: EVENT_FALL}.get(direction)
        if d is None:
            raise ValueError(f"direction must be 'rise' or 'fall', not {direction!r}")
        return d

    def times(self, direction, level=0):
        """``(t, t_last)``: the sub-sample times of the first E events of ``direction`` (``"rise"`` or ``"fall"``) at
        ``level``, (N, nrows, E), NaN where a slot is empty, and the last event's time (N, nrows), NaN where there was none"""
        d = self._direction(direction)
        m = self.idx[:, :, level, d, :].astype(np.float64)
        a, b = self.ab[:, :, level, d, :, 0], self.ab[:, :, level, d, :, 1]
        thr = (self.hi if d == EVENT_RISE else self.lo)[level][:, None, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(np.isnan(a), m, (m - 1.0) + (thr - a) / (b - a))
        t = np.where(self.idx[:, :, level, d, :] < 0, np.nan, t)
        return t[..., :-1], t[..., -1]

    def frequency(self, fs, level=0):
        """the frequency of an oscillating row from its rises at ``level`` (N, nrows): ``(n - 1) / (t_last - t_first) fs``, NaN
        with fewer than two rises (or with ``slots == 0``: the first rise is not recorded)"""
        t, last = self.times("rise", level)
        n = self.rises[:, :, level].astype(np.float64)
        if t.shape[-1] == 0:
            return np.full(n.shape, np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n >= 2, (n - 1.0) / (last - t[..., 0]) * fs, np.nan)

    def duty(self, level=0):
        """the share of the decided samples the row spends HIGH at ``level`` (N, nrows): ``HIGH / (HIGH + LOW)``"""
        h, l = self.high[:, :, level].astype(np.float64), self.low[:, :, level].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return h / (h + l)

    def transition_time(self, level_a, level_b, direction="rise"):
        """the first event of ``direction`` at ``level_b`` minus the first at ``level_a``, in samples (N, nrows): the rise
        time between a 10 % and a 90 % level; NaN where either has none (needs ``slots >= 1``)"""
        ta, tb = self.times(direction, level_a)[0], self.times(direction, level_b)[0]
        if ta.shape[-1] == 0:
            return np.full(ta.shape[:2], np.nan)
        return tb[..., 0] - ta[..., 0]

    def last_time(self, level=0):
        """the later of the last rise and the last fall at ``level`` (N, nrows), NaN where there was neither: with two levels
        that bracket the final value, the settling time out of the band"""
        return np.fmax(self.times("rise", level)[1], self.times("fall", level)[1])

    @classmethod
    def concatenate(cls, parts):
        """several batches' results (the shards of ``MultiDeviceRunner``) as one, along the instances"""
        a = parts[0]
        if any((p.count, p.rows, p.levels, p.slots) != (a.count, a.rows, a.levels, a.slots) for p in parts):
            raise ValueError("the shards' events differ in their sample counts, measured rows, levels or slots")
        cat = lambda k, axis=0: np.concatenate([getattr(p, k) for p in parts], axis=axis)
        return cls(cat("counts"), cat("idx"), cat("ab"), a.count, cat("lo", 1), cat("hi", 1), a.rows)


class MeasurementWeighting:
    """What ``ModelRunner.measurement_weighting()`` returns, and what ``set_measurement_weighting`` accepts: a cascade of
    second-order sections, ``sos`` (S, 5) with the rows ``b0 b1 b2 a1 a2`` of
    H(z) = (b0 + b1 z^-1 + b2 z^-2) / (1 + a1 z^-1 + a2 z^-2)."""

    def __init__(self, sos):
        self.sos = sos_rows(sos)

    def apply(self, x):
        """the cascade on ``x`` along its last axis from rest, in the arithmetic of ``acme_batch_set_measurement_weighting``
        (transposed direct form II, every product and sum rounded on its own): bit for bit what the device's measurement
        reads for an output ``x``.  Weight a target recording with it before ``set_measurement_target``."""
        x = np.array(x, dtype=np.float64)
        w = np.empty_like(x)
        s1 = np.zeros((len(self.sos),) + x.shape[:-1])
        s2 = np.zeros_like(s1)
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(x.shape[-1]):
                v = x[..., t]
                for k, (b0, b1, b2, a1, a2) in enumerate(self.sos):
                    xk = v
                    v = b0 * xk + s1[k]
                    s1[k] = (b1 * xk - a1 * v) + s2[k]
                    s2[k] = b2 * xk - a2 * v
                w[..., t] = v
        return w

    def response(self, f, fs):
        """the complex frequency response at the frequencies ``f`` (Hz) for the sample rate ``fs``"""
        z1 = np.exp(-2j * np.pi * np.asarray(f, dtype=np.float64) / fs)
        h = np.ones_like(z1)
        for b0, b1, b2, a1, a2 in self.sos:
            h = h * ((b0 + b1 * z1 + b2 * z1 * z1) / (1.0 + a1 * z1 + a2 * z1 * z1))
        return h


def sos_rows(sos):
    """second-order sections as the ABI takes them, (S, 5) ``b0 b1 b2 a1 a2``: from (S, 5), or from scipy's (S, 6)
    ``b0 b1 b2 a0 a1 a2`` whose ``a0`` must be 1.0 exactly"""
    if isinstance(sos, MeasurementWeighting):
        return sos.sos
    a = np.asarray(sos, dtype=np.float64)
    if a.ndim == 1 and a.shape[0] in (5, 6):
        a = a[None]
    if a.ndim != 2 or a.shape[1] not in (5, 6) or not 1 <= a.shape[0] <= MAX_WEIGHTING_SECTIONS:
        raise DimensionMismatch(f"second-order sections must have shape (S, 5) or (S, 6), S = 1 ... {MAX_WEIGHTING_SECTIONS}")
    if a.shape[1] == 6:
        if not np.all(a[:, 3] == 1.0):
            raise ValueError("second-order sections in the six-column layout must have a0 == 1.0 (normalise them first)")
        a = a[:, [0, 1, 2, 4, 5]]
    return np.ascontiguousarray(a)


def _bilinear_section(num, den, fs):
    """(n2, n1, n0) / (d2, d1, d0) in s -> b0 b1 b2 a1 a2 by s = 2 fs (1 - z^-1) / (1 + z^-1), no pre-warping"""
    c = 2.0 * fs
    poly = lambda n2, n1, n0: np.array([n2 * c * c + n1 * c + n0, 2.0 * n0 - 2.0 * n2 * c * c, n2 * c * c - n1 * c + n0])
    b, a = poly(*num), poly(*den)
    return np.concatenate([b / a[0], a[1:] / a[0]])


# IEC 61672-1: the poles of the A and C weightings (Hz)
_F1, _F2, _F3, _F4 = 20.598997, 107.65265, 737.86223, 12194.217


def weighting_sos(kind, fs, r=0.995):
    """Second-order sections (S, 5) for ``set_measurement_weighting`` at the sample rate ``fs``:

    ``"A"``, ``"C"``  the IEC 61672 frequency weightings: the plain bilinear transform of the analog poles (20.6 Hz and
               12 194 Hz double, for A also 107.7 Hz and 737.9 Hz), WITHOUT pre-warping, scaled to |H| = 1 at 1 kHz.  S = 3 / 2.
    ``"K"``    the pre-filter of ITU-R BS.1770: the high shelf and the high-pass from their analog parameters by the usual
               tan(pi f0 / fs) formulas; at 48 kHz the standard's coefficient tables.  S = 2.
    ``"dc"``   the DC blocker (1 - z^-1) / (1 - r z^-1).  S = 1.

    What the plain bilinear transform costs near Nyquist: the response at f is the analog one at (fs / pi) tan(pi f / fs),
    so at 44.1 kHz the A curve reads -4.0 dB at 10 kHz where the analog curve reads -2.5 dB (48 kHz: -3.7 dB); below a few
    kHz the two agree closely.  A caller who needs the analog curve to the top of the band brings a design of their own --
    any (S, 5) or scipy-layout (S, 6) array is accepted."""
    fs = float(fs)
    if kind in ("A", "C"):
        w1, w2, w3, w4 = (2.0 * np.pi * f for f in (_F1, _F2, _F3, _F4))
        secs = [_bilinear_section((1.0, 0.0, 0.0), (1.0, 2.0 * w1, w1 * w1), fs)]
        if kind == "A":
            secs.append(_bilinear_section((1.0, 0.0, 0.0), (1.0, w2 + w3, w2 * w3), fs))
        secs.append(_bilinear_section((0.0, 0.0, 1.0), (1.0, 2.0 * w4, w4 * w4), fs))
        sos = np.array(secs)
        sos[0, :3] /= abs(MeasurementWeighting(sos).response(1000.0, fs))
        return sos
    if kind == "K":
        f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
        K = np.tan(np.pi * f0 / fs)
        Vh = 10.0 ** (G / 20.0)
        Vb = Vh ** 0.4996667741545416
        a0 = 1.0 + K / Q + K * K
        shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
                 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
        f0, Q = 38.13547087602444, 0.5003270373238773
        K = np.tan(np.pi * f0 / fs)
        a0 = 1.0 + K / Q + K * K
        return np.array([shelf, [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]])
    if kind == "dc":
        return np.array([[1.0, -1.0, 0.0, -float(r), 0.0]])
    raise ValueError('weighting_sos: kind must be "A", "C", "K" or "dc"')


def segment_window(nfft, window):
    """the ``window`` argument of ``set_measurement_spectrum`` / ``set_measurement_cross`` as the ABI takes it: "hann" (periodic),
    "rect" (None: all ones) or ``nfft`` values"""
    if isinstance(window, str):
        if window == "hann":
            return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(max(nfft, 0)) / max(nfft, 1))
        if window == "rect":
            return None
        raise ValueError(f"window {window!r}: \"hann\", \"rect\" or an array of nfft values")
    w = np.ascontiguousarray(window, dtype=np.float64)
    if w.shape != (nfft,):
        raise DimensionMismatch(f"the window needs {nfft} values")
    return w


def measure_spec(ny, start=0, length=0, f0=None, harmonics=0, rows=None):
    """((start, length, f_num, f_den, harmonics, row mask), measured rows) -- acme_batch_set_measurement's arguments -- from
    ``ModelRunner.set_measurement``'s: ``f0`` a Fraction of fs or
    (num, den); ``rows`` the output rows to measure (None: all)."""
    from fractions import Fraction
    if f0 is None:
        if harmonics:
            raise ValueError("harmonics need a fundamental f0")
        num, den = 0, 1
    elif isinstance(f0, tuple):
        num, den = (int(v) for v in f0)
    else:
        f = Fraction(f0)
        num, den = f.numerator, f.denominator
    mask = 0
    rows = list(range(min(ny, 64))) if rows is None else sorted(set(int(r) for r in rows))
    for r in rows:
        if r < 0 or r >= 64:          # (the mask has 64 bits; the library refuses rows beyond the model's outputs)
            raise DimensionMismatch(f"output row {r}: rows 0 ... 63 can be measured")
        mask |= 1 << r
    return (int(start), int(length), num, den, int(harmonics), mask if rows else 0), rows


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _fa(a):
    return np.asfortranarray(a, dtype=np.float64)


class _ModelHandle:
    """acme_model* built from a DiscreteModel."""

    def __init__(self, lib, model):
        self.lib = lib
        h = C.c_void_p()
        keep = [_fa(model.a), _fa(model.b), _fa(model.c), _fa(model.x0), _fa(model.dy),
                _fa(model.ey), _fa(model.fy), _fa(model.y0)]
        lib.check(lib.L.acme_model_create(model.nx, model.nu, model.ny, model.nn_total,
                                          *[_dp(k) for k in keep], C.byref(h)))
        self.h = h
        for k, s in enumerate(model.subs):
            kind, qoff, roff, par = s.elem_arrays()
            mats = [_fa(s.pexp), _fa(s.dq), _fa(s.eq), _fa(s.fqprev), _fa(s.fq), _fa(s.q0),
                    _fa(s.init_z)]
            par = np.ascontiguousarray(par)
            lib.check(lib.L.acme_model_add_subproblem(
                h, s.nn, s.nq, s.np, *[_dp(k) for k in mats], len(s.table), _ip(kind),
                _ip(qoff), _ip(roff), _dp(par)))
            if s.row_order is not None:
                ro = np.ascontiguousarray(s.row_order, dtype=np.int32)
                lib.check(lib.L.acme_model_set_row_order(h, k, _ip(ro), len(ro)))

    def kernel_shape(self):
        dims = (C.c_int * 6)()
        self.lib.check(self.lib.L.acme_model_kernel_shape(self.h, dims))
        return tuple(dims)

    def kernel_variant(self):
        """(condensed_rows, generic): rows eliminated ahead of the Newton iteration, run-time-sized kernel"""
        nl, gen = C.c_int(0), C.c_int(0)
        self.lib.check(self.lib.L.acme_model_kernel_variant(self.h, C.byref(nl), C.byref(gen)))
        return nl.value, bool(gen.value)

    def kernel_family(self):
        """"tuned" (an instantiated shape), "coop" (run-time-sized, one instance per 16 lanes, working arrays in LDS:
        csrc/acme_coop.h) or "generic" (run-time-sized, one lane per instance: csrc/acme_generic.h)"""
        gen = C.c_int(0)
        self.lib.check(self.lib.L.acme_model_kernel_variant(self.h, None, C.byref(gen)))
        return ("tuned", "generic", "coop")[gen.value]

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.L.acme_model_destroy(self.h)
            self.h = None


def _print_progress(done, total):
    import sys
    sys.stderr.write("\rrun!: %3d %% (%d / %d samples)%s" % (100 * done // max(total, 1), done, total, "\n" if done >= total else ""))
    sys.stderr.flush()


class ModelRunner:
    """``ModelRunner(model, showprogress)`` for ``n_instances`` parallel copies of a model.

    ``models``: optional list of ``n_instances`` DiscreteModels with the same circuit
    topology but different component values (per-instance matrices, e.g. Monte-Carlo
    component tolerances); the element tables must be identical.
    """

    def __init__(self, model, n_instances=1, showprogress=False, device=None, models=None,
                 lib=None, maxiter=None):
        if not isinstance(model, DiscreteModel):
            raise TypeError("model must be a DiscreteModel")
        self.lib = lib or default_library()
        if self.lib.device_count() <= 0:
            raise AcmeError("no HIP device available; acme_jl_amd has no CPU fallback")
        self.model = model
        self.n = int(n_instances)
        # ``showprogress``: True prints a progress line per time slice of a host-buffer run (the reference wraps
        # its sample loop in @showprogress, src/ACME.jl:587-604,653); a callable gets (samples_done, samples_total)
        self.showprogress = showprogress
        self._mh = _ModelHandle(self.lib, model)
        o = Options()
        self.lib.L.acme_default_options(C.byref(o))
        o.solver = SOLVER_IDS[model.solver]
        o.device = -1 if device is None else int(device)
        o.per_instance_matrices = 1 if models is not None else 0
        if maxiter is not None:         # Newton iterations per base solve (``Options.maxiter``; None: the library's default)
            o.maxiter = int(maxiter)
        h = C.c_void_p()
        self.lib.check(self.lib.L.acme_batch_create(self._mh.h, self.n, C.byref(o), C.byref(h)))
        self.h = h
        self._warned = 0
        self._os = (1, 1, 1)            # oversampling: factor, interpolation taps, decimation taps
        self._meas = None               # measurement: (harmonics, measured rows) while armed
        self._series = (0, None)        # (the armed start, (win, hop, windows) of a series or None)
        self._fold = False              # a fold is set on the armed measurement
        self._spectrum = None           # (nfft, hop) of the spectrum set on the armed measurement
        self._cross = None              # (nfft, hop, in_row) of the cross-spectrum set on the armed measurement
        self._target = False            # a target is set on the armed measurement
        self._weighting = False         # a weighting is set on the armed measurement
        self._ensemble = None           # (G, stride, E) of the ensemble set on the armed measurement
        self._histogram = None          # (B, mode) of the histogram set on the armed measurement
        self._events = None             # (C, E, lo, hi) of the events set on the armed measurement
        self._length = 0                # the armed measurement's window length (0: unbounded)
        self._sources = {}              # input row -> kind, while the row has a source
        self._sine = {}                 # input row -> (f_den, f_num as armed) of its sine source
        self._progress_cb = None
        if showprogress:
            fn = showprogress if callable(showprogress) else _print_progress
            self._progress_cb = PROGRESS_FN(lambda user, done, total: fn(int(done), int(total)))    # (kept alive here)
            self.lib.check(self.lib.L.acme_batch_set_progress_callback(self.h, self._progress_cb, None))
        if models is not None:
            self.set_models(0, models)

    def set_isolation(self, iters_per_sample):
        """Run the instances that needed more than ``iters_per_sample`` Newton iterations per sample over the previous
        run in a launch of their own (``acme_batch_set_isolation``): device-pointer runs then complete on the caller's
        stream for the others, ``wait()`` completes the slow ones.  0 switches it off."""
        self.lib.check(self.lib.L.acme_batch_set_isolation(self.h, float(iters_per_sample)))

    def set_oversampling(self, factor, up=None, down=None, held_rows=()):
        """Oversampled runs (``acme_batch_set_oversampling``): the model -- derived at ``factor`` x the signal rate -- runs
        ``factor`` samples per sample of u / y, which every ``run*`` method takes and returns at the BASE rate.  Input rows
        are interpolated with ``factor * up`` (zero-stuffed), ``held_rows`` held (zero-order hold; the constant rows of
        ``run_const`` always are), the outputs decimated with ``down``; ``None`` = the library's default lowpass
        (``design_oversampling_filter``).  The histories of the filters are reset: each signal's first sample extends into
        the past at the next run, later runs continue where the last ended.  Reports count model-rate samples.
        ``factor=1`` switches it off."""
        def taps(h):
            if h is None:
                return None, None, 0
            a = np.ascontiguousarray(np.asarray(h, dtype=np.float64).ravel())
            return a, _dp(a), len(a)
        mask = 0
        for r in held_rows:
            r = int(r)
            if r < 0 or r >= 64:          # (the mask has 64 bits; the library refuses rows beyond the model's inputs)
                raise DimensionMismatch(f"held row {r}: rows 0 ... 63 can be held")
            mask |= 1 << r
        ua, up_p, nu_ = taps(up)
        da, dn_p, nd_ = taps(down)
        self.lib.check(self.lib.L.acme_batch_set_oversampling(self.h, int(factor), up_p, nu_, dn_p, nd_, mask))
        lu = nu_ if up is not None else len(design_oversampling_filter(factor, self.lib))
        ld = nd_ if down is not None else len(design_oversampling_filter(factor, self.lib))
        self._os = (int(factor), lu, ld)
        return self

    @property
    def oversampling(self):
        """the batch's oversampling factor (1: off)"""
        return self._os[0]

    @property
    def oversampling_delay(self):
        """base-rate samples by which the interpolation and decimation filters delay the signal (linear-phase filters:
        ((Lu - 1) + (Ld - 1)) / (2 factor); the default pair: the whole number (L - 1) / factor); 0 without oversampling"""
        k, lu, ld = self._os
        if k == 1:
            return 0
        d = ((lu - 1) + (ld - 1)) / (2 * k)
        return int(d) if d == int(d) else d

    # ---- output measurements ------------------------------------------------------------------
    def set_measurement(self, start=0, length=0, f0=None, harmonics=0, rows=None, f_den=None, f_num=None, f0_from_source=None):
        """Arm an output measurement (``acme_batch_set_measurement``): from now on every run feeds per instance and output
        row (``rows``: which, None = all) the mean, RMS, min, max and the complex amplitudes of ``harmonics`` harmonics of
        the fundamental ``f0`` -- a ``Fraction`` of fs or ``(num, den)`` -- over the samples ``start <= n < start + length``
        counted from now (``length=0``: all from ``start`` on).  ``measure`` then runs without storing y at all.

        A fundamental PER INSTANCE (``acme_batch_set_measurement_per_instance``) instead of ``f0``: ``f_den`` with ``f_num``,
        a scalar or N integers -- instance i correlates with f_num[i] / f_den of the sample rate --, or
        ``f0_from_source=row``: the ``f_den`` / ``f_num`` of the sine source (or the burst source's tone) armed on input row ``row`` (``set_source``).  A
        window of ``length=f_den`` samples holds whole periods of every instance's fundamental."""
        if f0_from_source is not None:
            if f0 is not None or f_num is not None or f_den is not None:
                raise ValueError("f0_from_source excludes f0 and f_den / f_num")
            src = self._sources.get(int(f0_from_source))
            if src not in (SOURCE_SINE, SOURCE_BURST):       # (a burst's tone is a sine's)
                raise ValueError(f"input row {f0_from_source} has no sine source to take the fundamental from")
            f_den, f_num = self._sine[int(f0_from_source)]
        if f_num is None and f_den is None:
            spec, rows = measure_spec(self.model.ny, start, length, f0, harmonics, rows)
            self.lib.check(self.lib.L.acme_batch_set_measurement(self.h, *spec))
        else:
            if f0 is not None:
                raise ValueError("f0 and f_den / f_num exclude each other: one fundamental, or one per instance")
            if f_num is None or f_den is None:
                raise ValueError("per-instance fundamentals need both f_den and f_num")
            spec, rows = measure_spec(self.model.ny, start, length, (0, int(f_den)), harmonics, rows)
            fa, fp = self._per_instance(f_num, np.int64, "f_num")
            self.lib.check(self.lib.L.acme_batch_set_measurement_per_instance(self.h, spec[0], spec[1], int(f_den), fp,
                                                                              spec[4], spec[5]))
        self._meas = (int(harmonics), rows)
        self._length = int(length)
        self._series = (int(start), None)
        self._fold = False
        self._spectrum = None
        self._cross = None
        self._target = False
        self._weighting = False
        self._ensemble = None
        self._histogram = None
        self._events = None
        return self

    def set_measurement_bins(self, coef, start=0, length=0, rows=None, f_den=None, f_num=None, tones_from_source=None):
        """Arm a measurement whose bins are integer combinations of per-instance tones
        (``acme_batch_set_measurement_bins``): ``coef`` (B, tones) integers, bin b of instance i at
        (sum_j coef[b][j] f_num[j][i]) mod f_den of ``f_den`` -- the sum and difference products of a two-tone test.
        ``f_num``: (tones, N) or (tones,) integers; or ``tones_from_source=row``: ``f_den`` and the tones of the multisine (or
        sine) source armed on input row ``row``.  ``measurement().bins`` then holds the complex amplitudes (N, nrows, B); a
        combination below zero reads the mirrored line (the conjugate amplitude): prefer signs that give a positive frequency."""
        if tones_from_source is not None:
            if f_num is not None or f_den is not None:
                raise ValueError("tones_from_source excludes f_den / f_num")
            if self._sources.get(int(tones_from_source)) not in (SOURCE_SINE, SOURCE_MULTISINE):
                raise ValueError(f"input row {tones_from_source} has no multisine or sine source to take the tones from")
            f_den, f_num = self._sine[int(tones_from_source)]
            f_num = np.atleast_2d(np.broadcast_to(f_num, (self.n,)) if np.ndim(f_num) < 2 else f_num)
        if f_num is None or f_den is None:
            raise ValueError("bins need f_den and f_num, or tones_from_source")
        fa, fp, tones = self._per_tone(f_num, np.int64, "f_num")
        ca = np.asarray(coef)
        if ca.size == 0:
            ca = np.zeros((0, tones), dtype=np.int32)
        if ca.ndim == 1 and tones == 1:
            ca = ca[:, None]
        if ca.ndim != 2 or ca.shape[1] != tones or not np.all(ca == np.round(ca)):
            raise DimensionMismatch(f"coef must be (bins, {tones}) integers")
        if np.abs(ca).max(initial=0) > 32767:
            raise ValueError("coef: |coefficient| <= 32767")
        ca = np.ascontiguousarray(ca, dtype=np.int32)
        spec, rows = measure_spec(self.model.ny, start, length, (0, int(f_den)), 0, rows)
        self.lib.check(self.lib.L.acme_batch_set_measurement_bins(self.h, spec[0], spec[1], int(f_den), tones, fp, ca.shape[0],
                                                                  _ip(ca), spec[5]))
        self._meas = (ca.shape[0], rows)
        self._length = int(length)
        self._series = (int(start), None)
        self._fold = False
        self._spectrum = None
        self._cross = None
        self._target = False
        self._weighting = False
        self._ensemble = None
        self._histogram = None
        self._events = None
        return self

    def measurement_plan(self):
        """The plan of the armed per-instance or bins measurement (``acme_batch_get_measurement_plan``): a dict with ``groups``
        (distinct f_num), ``chunk`` (samples per step), ``perm`` (lane slot -> pair) and ``wave_group`` (per wave of 64
        slots its one group -- the broadcast loop --, or -1: a mixed wave of per-lane loads)."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        P = self.n * len(self._meas[1])
        perm, wg = np.zeros(P, dtype=np.int64), np.zeros((P + 63) // 64, dtype=np.int32)
        F, chunk = C.c_longlong(0), C.c_longlong(0)
        self.lib.check(self.lib.L.acme_batch_get_measurement_plan(
            self.h, C.byref(F), C.byref(chunk), perm.ctypes.data_as(C.POINTER(C.c_longlong)), _ip(wg)))
        return dict(groups=F.value, chunk=chunk.value, perm=perm, wave_group=wg)

    def clear_measurement(self):
        """switch the measurement off (``acme_batch_clear_measurement``)"""
        self.lib.check(self.lib.L.acme_batch_clear_measurement(self.h))
        self._meas = None
        self._series = (0, None)
        self._fold = False
        self._spectrum = None
        self._cross = None
        self._target = False
        self._weighting = False
        self._ensemble = None
        self._histogram = None
        self._events = None
        return self

    def set_measurement_series(self, win, hop=None, windows=1):
        """Turn the armed measurement's one window into a series (``acme_batch_set_measurement_series``): ``windows`` windows
        of ``win`` samples, one every ``hop`` samples (None: ``win``, back to back), window w over
        ``start + w hop <= n < start + w hop + win`` -- all accumulated in the same pass, each bit for bit the single window
        armed there.  Needs a measurement armed with ``length=0`` that has not been fed yet; ``measurement_series`` reads it."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        hop = win if hop is None else hop
        self.lib.check(self.lib.L.acme_batch_set_measurement_series(self.h, int(win), int(hop), int(windows)))
        self._series = (self._series[0], (int(win), int(hop), int(windows)))
        return self

    def measurement_series(self, first=0, n=None):
        """the windows ``first ... first + n - 1`` (None: to the last) of the series so far
        (``acme_batch_get_measurement_series``): a ``MeasurementSeries``"""
        if self._meas is None or self._series[1] is None:
            raise AcmeError("no measurement series is set")
        (H, rows), (start, (win, hop, W)) = self._meas, self._series
        n = W - int(first) if n is None else int(n)
        out = np.empty((max(n, 0), self.n, len(rows), 4 + 2 * H))
        counts = np.zeros(max(n, 0), dtype=np.int64)
        self.lib.check(self.lib.L.acme_batch_get_measurement_series(self.h, int(first), n, _dp(out),
                                                                    counts.ctypes.data_as(C.POINTER(C.c_longlong))))
        return MeasurementSeries(out, counts, rows, start, win, hop, first)

    def set_measurement_fold(self, period=None, period_from_source=None):
        """Fold the armed measurement's window onto one period (``acme_batch_set_measurement_fold``, synchronous averaging):
        slot ``m mod period`` of the window-relative sample m accumulates y, per instance and measured row -- the steady
        state's waveform itself in place of y.  ``period``: samples, an int or N ints (one per instance), 1 ... 65536; or
        ``period_from_source=row``: the period of the sine or multisine source armed on input row ``row``,
        ``f_den // gcd(f_den, f_num[i])`` per instance (a multisine: the least common multiple over its tones).  Needs an
        armed measurement (any form, any window) that has not been fed yet; not together with a series;
        ``measurement_fold`` reads it."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        if (period is None) == (period_from_source is None):
            raise ValueError("a fold needs period or period_from_source")
        if period_from_source is not None:
            row = int(period_from_source)
            if self._sources.get(row) not in (SOURCE_SINE, SOURCE_MULTISINE):
                raise ValueError(f"input row {row} has no sine or multisine source to take the period from")
            f_den, f_num = self._sine[row]
            tones = np.atleast_2d(np.broadcast_to(f_num, (self.n,)) if np.ndim(f_num) < 2 else f_num).astype(np.int64)
            period = np.lcm.reduce(f_den // np.gcd(f_den, tones), axis=0)
            if period.max() > MAX_FOLD_PERIOD:
                i = int(period.argmax())
                raise ValueError(f"the source's period of instance {i}, {int(period[i])} samples, exceeds {MAX_FOLD_PERIOD}")
        if np.ndim(period) == 0:
            self.lib.check(self.lib.L.acme_batch_set_measurement_fold(self.h, int(period), None))
        else:
            pa, pp = self._per_instance(period, np.int64, "period")
            if np.shape(period) != (self.n,):
                raise DimensionMismatch(f"per-instance periods need {self.n} values")
            self.lib.check(self.lib.L.acme_batch_set_measurement_fold(self.h, 0, pp))
        self._fold = True
        return self

    def measurement_fold(self, raw=False):
        """the fold so far (``acme_batch_get_measurement_fold``): a ``MeasurementFold``.  ``raw``: ``mean`` holds the slots'
        sums, undivided (``acme_batch_get_measurement_fold_sums``; the tests pin the chains on them)."""
        if self._meas is None or not self._fold:
            raise AcmeError("no measurement fold is set")
        lp = C.POINTER(C.c_longlong)
        period, count = np.zeros(self.n, dtype=np.int64), C.c_longlong(0)
        self.lib.check(self.lib.L.acme_batch_get_measurement_fold(self.h, None, period.ctypes.data_as(lp), C.byref(count)))
        rows = self._meas[1]
        out = np.empty((self.n, len(rows), int(period.max(initial=0))))
        if raw:
            self.lib.check(self.lib.L.acme_batch_get_measurement_fold_sums(self.h, _dp(out)))
        else:
            self.lib.check(self.lib.L.acme_batch_get_measurement_fold(self.h, _dp(out), None, None))
        return MeasurementFold(out, period, count.value, rows)

    def set_measurement_spectrum(self, nfft, hop=None, window="hann"):
        """Welch-averaged periodograms of the armed measurement's window (``acme_batch_set_measurement_spectrum``): segments
        of ``nfft`` samples (a power of two, 64 ... 4096), one every ``hop`` (None: ``nfft // 2``), each multiplied by
        ``window`` -- "hann" (periodic), "rect" or ``nfft`` values --, transformed on the device and |X_k|^2 accumulated per
        instance, measured row and bin.  Needs an armed measurement (any form, any window) that has not been fed yet; not
        together with a series; ``measurement_spectrum`` reads it."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        nfft = int(nfft)
        hop = nfft // 2 if hop is None else int(hop)
        w = segment_window(nfft, window)
        self.lib.check(self.lib.L.acme_batch_set_measurement_spectrum(self.h, nfft, hop, None if w is None else _dp(w)))
        self._spectrum = (nfft, hop)
        return self

    def measurement_spectrum_table(self):
        """(w (nfft,), tw (nfft / 2, 2)): the window and the twiddles (cos, -sin)(2 pi k / nfft) the kernel uses
        (``acme_batch_get_measurement_spectrum_table``)"""
        if self._meas is None or self._spectrum is None:
            raise AcmeError("no measurement spectrum is set")
        nfft = self._spectrum[0]
        w, tw = np.empty(nfft), np.empty((nfft // 2, 2))
        self.lib.check(self.lib.L.acme_batch_get_measurement_spectrum_table(self.h, _dp(w), _dp(tw)))
        return w, tw

    def measurement_spectrum(self, raw=False):
        """the spectrum so far (``acme_batch_get_measurement_spectrum``): a ``MeasurementSpectrum``.  ``raw``: ``power`` holds
        the bins' sums, undivided (``acme_batch_get_measurement_spectrum_sums``; the tests pin the chains on them)."""
        if self._meas is None or self._spectrum is None:
            raise AcmeError("no measurement spectrum is set")
        nfft, hop = self._spectrum
        rows = self._meas[1]
        seg, count = C.c_longlong(0), C.c_longlong(0)
        out = np.empty((self.n, len(rows), nfft // 2 + 1))
        self.lib.check(self.lib.L.acme_batch_get_measurement_spectrum(self.h, None if raw else _dp(out), C.byref(seg), C.byref(count)))
        if raw:
            self.lib.check(self.lib.L.acme_batch_get_measurement_spectrum_sums(self.h, _dp(out)))
        return MeasurementSpectrum(out, seg.value, count.value, rows, self.measurement_spectrum_table()[0], hop)

    def set_measurement_cross(self, in_row, nfft, hop=None, window="hann"):
        """The cross-spectrum of input row ``in_row`` and the measured output rows over the armed measurement's window
        (``acme_batch_set_measurement_cross``): segments of ``nfft`` samples (a power of two, 64 ... 4096), one every ``hop``
        (None: ``nfft // 2``), each multiplied by ``window`` -- "hann" (periodic), "rect" or ``nfft`` values --; the input
        row, as the run sees it at the base rate (the caller's u, a constant row or a source), and a measured row go
        through one complex transform on the device, and |X|^2, |Y|^2 and conj(X) Y are accumulated per instance, measured
        row and bin.  Needs an armed measurement (any form, any window) that has not been fed yet; not together with a
        series; ``measurement_cross`` reads it."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        nfft = int(nfft)
        hop = nfft // 2 if hop is None else int(hop)
        w = segment_window(nfft, window)
        self.lib.check(self.lib.L.acme_batch_set_measurement_cross(self.h, int(in_row), nfft, hop, None if w is None else _dp(w)))
        self._cross = (nfft, hop, int(in_row))
        return self

    def measurement_cross_table(self):
        """(w (nfft,), tw (nfft / 2, 2)): the window and the twiddles (cos, -sin)(2 pi k / nfft) the kernel uses
        (``acme_batch_get_measurement_cross_table``)"""
        if self._meas is None or self._cross is None:
            raise AcmeError("no measurement cross-spectrum is set")
        nfft = self._cross[0]
        w, tw = np.empty(nfft), np.empty((nfft // 2, 2))
        self.lib.check(self.lib.L.acme_batch_get_measurement_cross_table(self.h, _dp(w), _dp(tw)))
        return w, tw

    def measurement_cross(self, raw=False):
        """the cross-spectrum so far (``acme_batch_get_measurement_cross``): a ``MeasurementCross``.  ``raw``: it holds the
        bins' sums, undivided (``acme_batch_get_measurement_cross_sums``; the tests pin the chains on them)."""
        if self._meas is None or self._cross is None:
            raise AcmeError("no measurement cross-spectrum is set")
        nfft, hop, in_row = self._cross
        rows = self._meas[1]
        seg, count = C.c_longlong(0), C.c_longlong(0)
        out = np.empty((self.n, len(rows), 4, nfft // 2 + 1))
        self.lib.check(self.lib.L.acme_batch_get_measurement_cross(self.h, None if raw else _dp(out), C.byref(seg), C.byref(count)))
        if raw:
            self.lib.check(self.lib.L.acme_batch_get_measurement_cross_sums(self.h, _dp(out)))
        sxy = np.empty(out[:, :, 2].shape, dtype=np.complex128)     # (the planes' bits: no arithmetic touches them)
        sxy.real, sxy.imag = out[:, :, 2], out[:, :, 3]
        return MeasurementCross(out[:, :, 0].copy(), out[:, :, 1].copy(), sxy, seg.value, count.value, rows, in_row,
                                self.measurement_cross_table()[0], hop)

    def set_measurement_target(self, target, which=None, lag=None, preemphasis=0.0):
        """Compare the armed measurement's window with a waveform of the caller's (``acme_batch_set_measurement_target``):
        per instance and measured row the sums of (y - t)^2, t^2, y t and t, the peak |y - t| and, behind the pre-emphasis
        filter 1 - ``preemphasis`` z^-1, the sums of the filtered error's and target's squares.  ``target``: (P,) -- one
        looped waveform for every measured row --, (nrows, P) or (K, nrows, P), K <= 64 recordings; ``which``: N integers
        (None: 0), the recording instance i is compared with; ``lag``: N integers 0 ... P - 1 (None: 0), instance i reads
        the target ``lag[i]`` samples ahead.  Needs an armed measurement (any form, any window) that has not been fed yet;
        not together with a series; ``measurement_target`` reads it."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        nrows = len(self._meas[1])
        t = np.asarray(target, dtype=np.float64)
        if t.ndim == 1:
            t = np.broadcast_to(t, (1, nrows, t.shape[0]))
        elif t.ndim == 2:
            t = t[None]
        if t.ndim != 3 or t.shape[1] != nrows:
            raise DimensionMismatch(f"the target must have shape (P,), ({nrows}, P) or (K, {nrows}, P)")
        t = np.ascontiguousarray(t)
        for a, what in ((which, "which"), (lag, "lag")):
            if a is not None and np.ndim(a) != 0 and np.shape(a) != (self.n,):
                raise DimensionMismatch(f"per-instance {what} needs {self.n} values")
        wa = None if which is None else np.ascontiguousarray(np.broadcast_to(np.asarray(which), (self.n,)), dtype=np.int32)
        if wa is not None and not np.all(wa == np.asarray(which)):
            raise DimensionMismatch("which must be integers")
        la, lp = self._per_instance(lag, np.int64, "lag")
        self.lib.check(self.lib.L.acme_batch_set_measurement_target(self.h, _dp(t), t.shape[0], t.shape[2],
                                                                    None if wa is None else _ip(wa), lp, float(preemphasis)))
        self._target = True
        return self

    def measurement_target(self, raw=False):
        """the residual against the target so far (``acme_batch_get_measurement_target``): a ``MeasurementTarget``.  ``raw``:
        the chains alone (``sums``; the tests pin them), without the read of the base measurement that ``error_mean`` needs."""
        if self._meas is None or not self._target:
            raise AcmeError("no measurement target is set")
        rows = self._meas[1]
        out, count = np.empty((self.n, len(rows), 7)), C.c_longlong(0)
        self.lib.check(self.lib.L.acme_batch_get_measurement_target(self.h, _dp(out), C.byref(count)))
        return MeasurementTarget(out, count.value, rows, None if raw else self.measurement().mean)

    def set_measurement_weighting(self, sos):
        """Put a cascade of second-order sections ahead of the armed measurement (``acme_batch_set_measurement_weighting``):
        every form -- the window's moments and harmonics, bins, a series, a fold, a spectrum, a cross-spectrum's output
        rows, a target's error -- then reads the weighted output, filtered from the first sample after arming on.  ``sos``:
        (S, 5) rows ``b0 b1 b2 a1 a2`` or scipy's (S, 6) with ``a0 == 1.0``, S <= 8, or a ``MeasurementWeighting``;
        ``weighting_sos`` makes the A, C and K curves and a DC blocker.  Needs an armed measurement that has not been fed
        yet; ``measurement_weighting`` reads it back."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        a = sos_rows(sos)
        self.lib.check(self.lib.L.acme_batch_set_measurement_weighting(self.h, _dp(a), a.shape[0]))
        self._weighting = True
        return self

    def measurement_weighting(self):
        """the weighting of the armed measurement (``acme_batch_get_measurement_weighting``): a ``MeasurementWeighting``"""
        if self._meas is None or not self._weighting:
            raise AcmeError("no measurement weighting is set")
        out, S = np.zeros((MAX_WEIGHTING_SECTIONS, 5)), C.c_int(0)
        self.lib.check(self.lib.L.acme_batch_get_measurement_weighting(self.h, _dp(out), C.byref(S)))
        return MeasurementWeighting(out[:S.value].copy())

    def set_measurement_ensemble(self, groups=None, n_groups=None, stride=1):
        """Reduce the armed measurement's window ACROSS the instances (``acme_batch_set_measurement_ensemble``): per group,
        measured row and recorded sample the sum, the sum of squares, the minimum and the maximum over the group's members
        and the instances that set the extremes -- the band of a Monte-Carlo batch with no y stored.  ``groups``: N integers,
        instance i's group 0 ... G - 1 or -1 (in none); None: every instance in group 0.  ``n_groups``: G (None: the
        largest group index + 1).  ``stride``: every ``stride``-th window sample is recorded.  Needs an armed measurement
        with a bounded window (``length > 0``) that has not been fed yet; not together with a series;
        ``measurement_ensemble`` reads it."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        ga = None
        if groups is not None:
            if np.shape(groups) != (self.n,):
                raise DimensionMismatch(f"groups needs {self.n} values")
            ga = np.ascontiguousarray(groups, dtype=np.int32)
            if not np.all(ga == np.asarray(groups)):
                raise DimensionMismatch("groups must be integers")
        G = int(n_groups) if n_groups is not None else 1 if ga is None else max(int(ga.max(initial=-1)) + 1, 1)
        stride = int(stride)
        self.lib.check(self.lib.L.acme_batch_set_measurement_ensemble(self.h, None if ga is None else _ip(ga), G, stride))
        self._ensemble = (G, stride, (self._length - 1) // stride + 1)
        return self

    def measurement_ensemble(self):
        """the statistics across the groups' instances so far (``acme_batch_get_measurement_ensemble``): a
        ``MeasurementEnsemble``"""
        if self._meas is None or self._ensemble is None:
            raise AcmeError("no measurement ensemble is set")
        rows = self._meas[1]
        G, stride, E = self._ensemble
        out, arg = np.empty((G, len(rows), E, 4)), np.empty((G, len(rows), E, 2), dtype=np.int64)
        members, filled = np.zeros(G, dtype=np.int64), C.c_longlong(0)
        lp = C.POINTER(C.c_longlong)
        self.lib.check(self.lib.L.acme_batch_get_measurement_ensemble(self.h, _dp(out), arg.ctypes.data_as(lp),
                                                                      members.ctypes.data_as(lp), C.byref(filled)))
        return MeasurementEnsemble(*(out[..., k].copy() for k in range(4)), arg[..., 0].copy(), arg[..., 1].copy(), members,
                                   filled.value, stride, rows)

    def set_measurement_histogram(self, bins, lo, hi, mode="signed"):
        """Count how the amplitude of every measured row is distributed (``acme_batch_set_measurement_histogram``): ``bins``
        equal bins over ``[lo, hi)`` per instance plus the samples below, at or above the range and not a number -- levels
        exceeded, percentiles and the density with no y stored.  ``lo``, ``hi``: scalars, or N values each (a scalar beside
        an array is repeated); ``mode``: ``"signed"`` or ``"abs"`` (the magnitude is binned).  Needs an armed measurement
        that has not been fed yet; not together with a series; ``measurement_histogram`` reads it."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        modes = {"signed": HIST_SIGNED, "abs": HIST_ABS, HIST_SIGNED: HIST_SIGNED, HIST_ABS: HIST_ABS}
        if mode not in modes:
            raise ValueError(f"mode must be 'signed' or 'abs', not {mode!r}")
        if np.ndim(lo) == 0 and np.ndim(hi) == 0:
            self.lib.check(self.lib.L.acme_batch_set_measurement_histogram(self.h, int(bins), modes[mode], float(lo), float(hi), None, None))
        else:
            for name, a in (("lo", lo), ("hi", hi)):
                if np.ndim(a) != 0 and np.shape(a) != (self.n,):
                    raise DimensionMismatch(f"{name} needs {self.n} values (or a scalar)")
            la = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (self.n,)))
            ha = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float64), (self.n,)))
            self.lib.check(self.lib.L.acme_batch_set_measurement_histogram(self.h, int(bins), modes[mode], 0.0, 0.0, _dp(la), _dp(ha)))
        self._histogram = (int(bins), "abs" if modes[mode] == HIST_ABS else "signed")
        return self

    def measurement_histogram(self):
        """the counters so far (``acme_batch_get_measurement_histogram``): a ``MeasurementHistogram``"""
        if self._meas is None or self._histogram is None:
            raise AcmeError("no measurement histogram is set")
        rows = self._meas[1]
        B, mode = self._histogram
        raw, rng, count = np.empty((self.n, len(rows), B + 3), dtype=np.int64), np.empty((self.n, 3)), C.c_longlong(0)
        self.lib.check(self.lib.L.acme_batch_get_measurement_histogram(self.h, raw.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(rng),
                                                                       C.byref(count)))
        return MeasurementHistogram(raw[..., 1:B + 1].copy(), raw[..., 0].copy(), raw[..., B + 1].copy(), raw[..., B + 2].copy(),
                                    count.value, rng[:, 0].copy(), rng[:, 1].copy(), rng[:, 2].copy(), mode, rows)

    def set_measurement_events(self, levels=None, hysteresis=0.0, slots=8, lo=None, hi=None):
        """Record when every measured row crosses levels (``acme_batch_set_measurement_events``): rise and fall times, delays,
        settling, frequency from zero crossings, duty cycle, chatter across a trip level, with no y stored.  ``levels``: a
        scalar, C values or (C, N) values, one row per level; each becomes the band ``level -+ hysteresis / 2`` (0.0: a plain
        comparator).  Or ``lo=`` and ``hi=`` explicitly, C or (C, N) values each, ``lo <= hi``.  ``slots``: the first events
        recorded per direction (the last one always is).  Needs an armed measurement that has not been fed yet; not together
        with a series; ``measurement_events`` reads it."""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        if (levels is None) == (lo is None and hi is None) or (lo is None) != (hi is None):
            raise ValueError("give either levels (with a hysteresis) or both lo and hi")
        if not hysteresis >= 0.0:
            raise ValueError("hysteresis must be >= 0")

        def full(a, name):
            a = np.asarray(a, dtype=np.float64)
            a = a.reshape(1, 1) if a.ndim == 0 else a[:, None] if a.ndim == 1 else a
            if a.ndim != 2 or a.shape[1] not in (1, self.n):
                raise DimensionMismatch(f"{name} needs C or (C, {self.n}) values")
            return np.ascontiguousarray(np.broadcast_to(a, (a.shape[0], self.n)))
        if levels is not None:
            mid = full(levels, "levels")
            la, ha = mid - 0.5 * hysteresis, mid + 0.5 * hysteresis
        else:
            la, ha = full(lo, "lo"), full(hi, "hi")
            if la.shape != ha.shape:
                raise DimensionMismatch("lo and hi need the same number of levels")
        self.lib.check(self.lib.L.acme_batch_set_measurement_events(self.h, la.shape[0], _dp(la), _dp(ha), int(slots)))
        self._events = (la.shape[0], int(slots), la, ha)
        return self

    def measurement_events(self):
        """the events so far (``acme_batch_get_measurement_events``): a ``MeasurementEvents``"""
        if self._meas is None or self._events is None:
            raise AcmeError("no measurement events are set")
        rows = self._meas[1]
        nC, E, la, ha = self._events
        lp = C.POINTER(C.c_longlong)
        counts = np.empty((self.n, len(rows), nC, 5), dtype=np.int64)
        idx = np.empty((self.n, len(rows), nC, 2, E + 1), dtype=np.int64)
        ab, count = np.empty((self.n, len(rows), nC, 2, E + 1, 2)), C.c_longlong(0)
        self.lib.check(self.lib.L.acme_batch_get_measurement_events(self.h, counts.ctypes.data_as(lp), idx.ctypes.data_as(lp), _dp(ab),
                                                                    C.byref(count)))
        return MeasurementEvents(counts, idx, ab, count.value, la.copy(), ha.copy(), rows)

    def reset_measurement(self):
        """zero the accumulators and restart the window's clock (``acme_batch_reset_measurement``)"""
        self.lib.check(self.lib.L.acme_batch_reset_measurement(self.h))
        return self

    def measurement(self):
        """the armed measurement's results so far (``acme_batch_get_measurement``): a ``Measurement``"""
        if self._meas is None:
            raise AcmeError("no measurement is armed")
        if self._series[1] is not None:
            raise AcmeError("the measurement has a series of windows: use measurement_series()")
        H, rows = self._meas
        out = np.empty((self.n, len(rows), 4 + 2 * H))
        count = C.c_longlong(0)
        self.lib.check(self.lib.L.acme_batch_get_measurement(self.h, _dp(out), C.byref(count)))
        return Measurement(out, count.value, rows)

    def measure(self, u=None, check=True, time_major=False, T=None):
        """``run`` without outputs: advance the instances over ``u`` (shapes as ``run``) and only feed the armed
        measurement (y = NULL: nothing of y is stored or copied).  Returns ``self``; ``measurement()`` reads the results.
        ``u=None`` when every input row has a source (``set_source``): ``T`` samples are generated on the device."""
        m = self.model
        if u is None:
            if T is None or len(self._sources) != m.nu:
                raise DimensionMismatch("measure(u=None) needs a source on every input row and the number of samples T")
            return self.run_sources(T, y=False, check=check)
        u = np.asarray(u, dtype=np.float64)
        if not time_major:
            if u.ndim == 2 and self.n == 1:
                u = u[None]
            if u.ndim != 3 or u.shape[0] != self.n or u.shape[1] != m.nu:
                raise DimensionMismatch(f"input must have shape ({self.n}, {m.nu}, T)")
            u = np.transpose(u, (0, 2, 1))
        if u.ndim != 3 or u.shape[0] != self.n or u.shape[2] != m.nu:
            raise DimensionMismatch(f"input must have shape ({self.n}, T, {m.nu})")
        ub = np.ascontiguousarray(u)
        self.lib.check(self.lib.L.acme_batch_run(self.h, ub.ctypes.data, None, ub.shape[1], ACME_MEM_HOST, None))
        self._hold(ub)
        if check:
            self.check()
        return self

    def measure_const(self, u_var, u_const, const_rows, check=True):
        """``run_const`` without outputs (y = NULL): only the armed measurement is fed.  Returns ``self``."""
        return self.run_const(u_var, u_const, const_rows, y=False, check=check)

    # ---- sources: input rows generated on the device ------------------------------------------
    def _per_instance(self, a, dtype, what):
        """a per-instance parameter (None, a scalar or N values) as the ABI takes it: (array kept alive, pointer)"""
        if a is None:
            return None, None
        arr = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=dtype), (self.n,)))
        if dtype is np.int64 and not np.all(arr == np.asarray(a)):
            raise DimensionMismatch(f"{what} must be integers")
        return arr, arr.ctypes.data_as(C.POINTER(C.c_double if dtype is np.float64 else C.c_longlong))

    def _per_tone(self, a, dtype, what, tones=None):
        """a per-tone, per-instance parameter -- (tones, N), (tones,) (one value per tone for every instance) or, with
        ``tones`` known, a scalar -- as the ABI takes it: (array kept alive, pointer, tones); None stays None"""
        if a is None:
            return None, None, tones
        src = np.asarray(a)
        if src.ndim == 0 and tones is not None:
            src = np.full((tones,), src)
        if src.ndim == 1:
            src = src[:, None]
        if src.ndim != 2 or src.shape[1] not in (1, self.n) or (tones is not None and src.shape[0] != tones):
            raise DimensionMismatch(f"{what} must have shape (tones, {self.n}) or (tones,)")
        arr = np.ascontiguousarray(np.broadcast_to(src.astype(dtype), (src.shape[0], self.n)))
        if dtype is np.int64 and not np.all(arr == src):
            raise DimensionMismatch(f"{what} must be integers")
        return arr, arr.ctypes.data_as(C.POINTER(C.c_double if dtype is np.float64 else C.c_longlong)), src.shape[0]

    def _pulse_shape(self, kind, period, delay, rise, on, fall, at):
        """the (5, N) integer block of a pulse or burst row -- period, delay, rise, on, fall, each a scalar or N values --;
        ``kind="step"``: P = 2^31 - 1, delay = at, on = P - at - rise"""
        if kind == "step":
            if period is not None or on is not None or delay is not None or fall is not None:
                raise ValueError("a step source takes at= and rise= (period, delay, on and fall are its own)")
            at_, rise_ = self._per_instance(0 if at is None else at, np.int64, "at")[0], self._per_instance(0 if rise is None else rise, np.int64, "rise")[0]
            period, delay, rise, on, fall = MAX_PULSE_PERIOD, at_, rise_, MAX_PULSE_PERIOD - at_ - rise_, 0
        elif at is not None:
            raise ValueError("at= belongs to a step source")
        elif period is None or on is None:
            raise ValueError("a pulse or burst source needs period and on")
        cols = [self._per_instance(0 if v is None else v, np.int64, what)[0]
                for v, what in ((period, "period"), (delay, "delay"), (rise, "rise"), (on, "on"), (fall, "fall"))]
        return np.ascontiguousarray(np.stack(cols))

    def set_source(self, row, kind, amp=None, offset=None, f_den=None, f_num=None, phase=None, table=None,
                   dist="gaussian", hold=1, stream=None, seed=0, period=None, delay=None, rise=None, on=None, fall=None, at=None):
        """Give input row ``row`` a source (``acme_batch_set_source_*``): the library generates the row on the device, at
        source clock n (base-rate samples since the first source was armed) for instance i

        * ``"const"``: ``offset[i]``
        * ``"sine"``: ``fma(amp[i], sin(2 pi kappa / f_den), offset[i])``, kappa = (f_num[i] n + phase[i]) mod f_den -- the
          frequency f_num[i] / f_den of the sample rate per instance, the phase reduced exactly in integers
        * ``"table"``: ``fma(amp[i], table[n mod P], offset[i])``, a looped wavetable of P entries
        * ``"multisine"``: a sum of 1 ... 4 sines, one fma chain in tone order from ``offset[i]``; ``f_num`` (required),
          ``phase``, ``amp``: (tones, N) or (tones,) -- per-instance tone frequencies, levels and relative phases (a two-tone
          intermodulation test); one tone is the ``"sine"`` row bit for bit
        * ``"noise"``: ``fma(amp[i], d, offset[i])`` with d an independent, reproducible random draw per (stream[i], row,
          n div hold) -- counter based (Philox4x32-10), so the value at clock n depends on nothing generated before, on no
          call boundary and on no device.  ``dist="uniform"``: d in (-1, 1), never 0, variance 1/3; ``dist="gaussian"``: d
          standard normal (Box-Muller, one draw per sample).  ``hold`` (1 ... 2^31 - 1): the draw is held over blocks of
          ``hold`` samples aligned to the clock (1: white noise; larger: stepped random values, a jumping pot).  ``stream``:
          N integers (equal streams on a row render equal sequences; the same stream on two rows independent ones);
          otherwise ``stream[i] = seed * 2^32 + i`` with ``0 <= seed < 2^31``
        * ``"pulse"``: ``fma(amp[i], e, offset[i])`` with e a per-instance trapezoid: ``period`` (1 ... 2^31 - 1), ``delay``
          (0 ... period - 1, default 0), ``rise``, ``on``, ``fall`` (>= 0, rise + on + fall <= period; rise and fall default 0),
          each a scalar or N integers; with j = (n - delay[i]) mod period[i], e = j / rise on the rising ramp, 1 for ``on``
          samples, (rise + on + fall - j) / fall on the falling ramp, 0 otherwise -- one division per ramp sample, so the row
          is pinned bit for bit.  rise = fall = 0: high for exactly ``on`` samples per period (duty on / period).  A PWM or
          duty sweep, an edge-time sweep, a delay scan are each one batch
        * ``"step"``: ``set_source(row, "step", at=d, rise=0, amp=, offset=)`` -- the pulse with period P = 2^31 - 1,
          delay = d, on = P - d - rise: ``offset`` before clock d, a ramp of ``rise`` samples, then ``offset + amp``; a long
          ``rise`` is a ramp-and-hold of a pot row.  It WRAPS at clock 2^31 - 1 + d (13.5 hours at 44.1 kHz)
        * ``"burst"``: a tone burst, ``g = amp[i] e`` then ``fma(g, sin(th), offset[i])`` with e the pulse's envelope (the same
          five keywords) and th the ``"sine"`` row's angle from ``f_den``, ``f_num``, ``phase`` (the TONE's phase): the sine row
          bit for bit where e = 1, ``offset`` where e = 0.  The tone runs with the clock, it does not restart per burst: a
          burst starts at a zero crossing when ``delay`` and ``period`` are multiples of the tone's period.  The row lends
          its frequency to ``set_measurement(f0_from_source=)`` as a sine row does

        On an oversampled batch an ideal edge (rise = 0 or fall = 0) wants its row in ``held_rows``.
        ``amp``, ``offset``, ``f_num``, ``phase``: None (amp 1, the others 0), a scalar or N values.  ``run_sources`` then runs
        without these rows; its results are those of ``run`` on ``render_sources``' array, bit for bit."""
        k = _SOURCE_KINDS.get(kind)
        if k is None:
            raise ValueError(f"unknown source kind {kind!r}: 'const', 'sine', 'multisine', 'table', 'noise', 'pulse', 'step' or 'burst'")
        oa, op = self._per_instance(offset, np.float64, "offset")
        L = self.lib.L
        if k in (SOURCE_PULSE, SOURCE_BURST):
            shape = self._pulse_shape("step" if kind == "step" else "pulse", period, delay, rise, on, fall, at)
            sp = shape.ctypes.data_as(C.POINTER(C.c_longlong))
            aa, ap = self._per_instance(amp, np.float64, "amp")
            if k == SOURCE_PULSE:
                self.lib.check(L.acme_batch_set_source_pulse(self.h, int(row), sp, ap, op))
                self._sine.pop(int(row), None)
            else:
                if f_den is None:
                    raise ValueError("a burst source needs f_den")
                fa, fp = self._per_instance(f_num, np.int64, "f_num")
                pa, pp = self._per_instance(phase, np.int64, "phase")
                self.lib.check(L.acme_batch_set_source_burst(self.h, int(row), sp, int(f_den), fp, pp, ap, op))
                self._sine[int(row)] = (int(f_den), 0 if fa is None else fa.copy())
            self._sources[int(row)] = k
            return self
        if any(v is not None for v in (period, delay, rise, on, fall, at)):
            raise ValueError("period, delay, rise, on, fall and at belong to a pulse, step or burst source")
        if k == SOURCE_NOISE:
            d = _NOISE_DISTS.get(dist)
            if d is None:
                raise ValueError(f"unknown noise distribution {dist!r}: 'gaussian' or 'uniform'")
            if int(hold) != hold:
                raise ValueError("a noise source's hold must be an integer")
            sa = noise_streams(self.n, stream, seed)
            aa, ap = self._per_instance(amp, np.float64, "amp")
            self.lib.check(L.acme_batch_set_source_noise(self.h, int(row), d, int(hold), sa.ctypes.data_as(C.POINTER(C.c_longlong)), ap, op))
            self._sine.pop(int(row), None)
            self._sources[int(row)] = k
            return self
        if k == SOURCE_MULTISINE:
            if f_den is None or f_num is None:
                raise ValueError("a multisine source needs f_den and f_num")
            fa, fp, tones = self._per_tone(f_num, np.int64, "f_num")
            if not 1 <= tones <= MAX_SOURCE_TONES:
                raise ValueError(f"a multisine source has 1 ... {MAX_SOURCE_TONES} tones")
            pa, pp, _ = self._per_tone(phase, np.int64, "phase", tones)
            aa, ap, _ = self._per_tone(amp, np.float64, "amp", tones)
            self.lib.check(L.acme_batch_set_source_multisine(self.h, int(row), int(f_den), tones, fp, pp, ap, op))
            self._sine[int(row)] = (int(f_den), fa.copy())
            self._sources[int(row)] = k
            return self
        aa, ap = self._per_instance(amp, np.float64, "amp")
        if k == SOURCE_CONST:
            self.lib.check(L.acme_batch_set_source_const(self.h, int(row), op))
        elif k == SOURCE_SINE:
            if f_den is None:
                raise ValueError("a sine source needs f_den")
            fa, fp = self._per_instance(f_num, np.int64, "f_num")
            pa, pp = self._per_instance(phase, np.int64, "phase")
            self.lib.check(L.acme_batch_set_source_sine(self.h, int(row), int(f_den), fp, pp, ap, op))
            self._sine[int(row)] = (int(f_den), 0 if fa is None else fa.copy())
        else:
            if table is None:
                raise ValueError("a table source needs a table")
            w = np.ascontiguousarray(np.asarray(table, dtype=np.float64).ravel())
            self.lib.check(L.acme_batch_set_source_table(self.h, int(row), _dp(w), len(w), ap, op))
        if k != SOURCE_SINE:
            self._sine.pop(int(row), None)
        self._sources[int(row)] = k
        return self

    def clear_source(self, row=-1):
        """the row is the caller's again (``acme_batch_clear_source``); ``row=-1``: every row"""
        self.lib.check(self.lib.L.acme_batch_clear_source(self.h, int(row)))
        if row < 0:
            self._sources, self._sine = {}, {}
        else:
            self._sources.pop(int(row), None)
            self._sine.pop(int(row), None)
        return self

    @property
    def source_clock(self):
        """the source clock: base-rate samples the source runs have advanced since the first source was armed"""
        n = C.c_longlong(0)
        self.lib.check(self.lib.L.acme_batch_get_source_clock(self.h, C.byref(n)))
        return n.value

    @source_clock.setter
    def source_clock(self, n):
        self.lib.check(self.lib.L.acme_batch_set_source_clock(self.h, int(n)))

    def _u_var(self, u_var, T):
        """(array or None, pointer, T): the rows without a source, (N, T, nu_var) in the ABI's layout"""
        nuv = self.model.nu - len(self._sources)
        if not self._sources:
            raise AcmeError("no input row has a source (set_source)")
        if nuv == 0:
            if u_var is not None and np.asarray(u_var).size:
                raise DimensionMismatch("every input row has a source: u_var must be None")
            if T is None:
                raise DimensionMismatch("every input row has a source: give the number of samples T")
            return None, None, int(T)
        if u_var is None:
            raise DimensionMismatch(f"u_var must have shape ({self.n}, T, {nuv})")
        u_var = np.ascontiguousarray(u_var, dtype=np.float64)
        if u_var.ndim != 3 or u_var.shape[0] != self.n or u_var.shape[2] != nuv or (T is not None and T != u_var.shape[1]):
            raise DimensionMismatch(f"u_var must have shape ({self.n}, T, {nuv})")
        return u_var, u_var.ctypes.data, u_var.shape[1]

    def run_sources(self, T=None, u_var=None, y=None, check=True):
        """``run`` with the sourced rows generated on the device (``acme_batch_run_sources``): ``u_var`` (N, T, nu_var) holds
        only the rows without a source, in row order -- None when every row has one, then ``T`` says how many samples.
        Returns y (N, T, ny); ``y=False`` while a measurement is armed: nothing of y is stored (returns ``self``)."""
        u_var, up, T = self._u_var(u_var, T)
        ny = self.model.ny
        if y is False:
            self.lib.check(self.lib.L.acme_batch_run_sources(self.h, up, None, T, ACME_MEM_HOST, None))
            self._hold(u_var)
            if check:
                self.check()
            return self
        if y is None:
            y = np.empty((self.n, T, ny), dtype=np.float64)
        elif not (isinstance(y, np.ndarray) and y.dtype == np.float64 and y.flags.c_contiguous and y.shape == (self.n, T, ny)):
            raise DimensionMismatch(f"y must be a C-contiguous float64 array of shape ({self.n}, {T}, {ny})")
        self.lib.check(self.lib.L.acme_batch_run_sources(self.h, up, y.ctypes.data, T, ACME_MEM_HOST, None))
        self._hold(u_var, y)
        if check:
            self.check()
        return y

    def run_sources_async(self, T=None, u_var=None, y=None):
        """``acme_batch_run_sources_async`` on host buffers (shapes as ``run_sources``; ``y=None`` while a measurement is
        armed: no outputs).  Returns at once; ``wait()`` joins the run.  The caller keeps ``y`` alive until then."""
        u_var, up, T = self._u_var(u_var, T)
        if y is not None and not (isinstance(y, np.ndarray) and y.dtype == np.float64 and y.flags.c_contiguous
                                  and y.shape == (self.n, T, self.model.ny)):
            raise DimensionMismatch(f"y must be a C-contiguous float64 array of shape ({self.n}, {T}, {self.model.ny})")
        self._inflight = (u_var, y)
        self._hold(u_var, y)
        self.lib.check(self.lib.L.acme_batch_run_sources_async(self.h, up, None if y is None else y.ctypes.data, T,
                                                               ACME_MEM_HOST, None))

    def render_sources(self, T=None, u_var=None):
        """The input (N, T, nu) a source run of ``T`` samples would feed from the current clock
        (``acme_batch_render_sources``): sourced rows generated, the others from ``u_var`` (zeros if None).  Advances
        neither the clock nor the model."""
        if u_var is None:
            if T is None:
                raise DimensionMismatch("render_sources needs T or u_var")
            up, T = None, int(T)
        else:
            u_var, up, T = self._u_var(u_var, T)
        out = np.empty((self.n, T, self.model.nu), dtype=np.float64)
        self.lib.check(self.lib.L.acme_batch_render_sources(self.h, up, out.ctypes.data, T, ACME_MEM_HOST, None))
        return out

    def set_balance(self, mode=-1):
        """Placement of the waves by their measured cost (``acme_batch_set_balance``): -1 the library decides
        (default), 0 off, 1 on.  Results do not depend on it (bit-identical)."""
        self.lib.check(self.lib.L.acme_batch_set_balance(self.h, int(mode)))
        return self

    def placement(self):
        """slot -> instance of the last launch (``acme_batch_get_placement``): -1 = empty slot; the identity while
        nothing is placed"""
        n = C.c_longlong(0)
        self.lib.check(self.lib.L.acme_batch_get_placement(self.h, None, C.byref(n)))
        out = np.empty(n.value, dtype=np.int32)
        self.lib.check(self.lib.L.acme_batch_get_placement(self.h, _ip(out), None))
        return out

    def set_host_retention(self, keep=True):
        """``acme_batch_set_host_retention``: promise that the host arrays handed to ``run_async`` / ``run(layout="abi")``
        stay allocated until others are passed, ``release_host_buffers()`` is called or the runner goes -- they are then
        page-locked once and runs are streamed at the device-resident rate.  Off by default: ``run`` works on per-call
        temporaries, which must never stay registered."""
        self.lib.check(self.lib.L.acme_batch_set_host_retention(self.h, 1 if keep else 0))
        self._retain = bool(keep)
        if not keep:
            self._held = None

    def release_host_buffers(self):
        """Un-page-lock the arrays of the last host-buffer run (``acme_batch_release_host_buffers``)."""
        self.lib.check(self.lib.L.acme_batch_release_host_buffers(self.h))
        self._held = None

    def _hold(self, *arrays):
        # a retaining runner keeps the arrays it handed to the library alive for as long as they may be page-locked:
        # until the next call's arrays replace them, release_host_buffers() or the batch's destruction
        if getattr(self, "_retain", False):
            self._held = arrays

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.L.acme_batch_destroy(self.h)       # (un-page-locks whatever is held: before the arrays go)
            self.h = None
        self._held = None

    # ---- per-instance matrices ----------------------------------------------------------
    def set_models(self, first, models, chunk=1024):
        """Give instances first.. their own model blocks (``acme_batch_set_matrices``); ``models``
        is any iterable of DiscreteModels, e.g. ``montecarlo.BatchModels``."""
        hs = []

        def flush():
            nonlocal first, hs
            if hs:
                arr = (C.c_void_p * len(hs))(*[m.h for m in hs])
                self.lib.check(self.lib.L.acme_batch_set_matrices(self.h, first, len(hs), arr))
                first += len(hs)
                hs = []
        for m in models:
            hs.append(_ModelHandle(self.lib, m))
            if len(hs) == chunk:
                flush()
        flush()

    # ---- run! ---------------------------------------------------------------------------
    def _check_io(self, u_rows, y_rows, ucols, ycols):
        m = self.model
        if u_rows != m.nu:
            raise DimensionMismatch(f"input matrix has {u_rows} rows, but model has {m.nu} inputs")
        if y_rows != m.ny:
            raise DimensionMismatch(f"output matrix has {y_rows} rows, but model has {m.ny} outputs")
        if ucols != ycols:
            raise DimensionMismatch(
                f"input matrix has {ucols} columns, output matrix has {ycols} columns")

    def run(self, u, y=None, check=True, time_major=False):
        """``run!(runner, u)`` / ``run!(runner, y, u)`` with numpy arrays.

        ``u``: (nu, T) for a single instance, else (N, nu, T); returns ``y`` of shape
        (ny, T) resp. (N, ny, T).  Raises like the reference when an instance hits a
        non-finite result and warns on convergence failures (unless ``check=False``).

        ``time_major=True``: ``u`` is (N, T, nu) and ``y`` (N, T, ny) -- the memory layout of the
        C ABI (and of Julia's nu x T matrices), passed through without the two transposing copies
        the default shapes cost when nu or ny exceed 1."""
        m = self.model
        u = np.asarray(u, dtype=np.float64)
        if time_major:
            if u.ndim != 3 or u.shape[0] != self.n:
                raise DimensionMismatch(f"input must have shape ({self.n}, T, {m.nu})")
            T = u.shape[1]
            if y is not None:
                if not (isinstance(y, np.ndarray) and y.dtype == np.float64 and y.flags.c_contiguous):
                    raise TypeError("y must be a C-contiguous float64 array")
                if y.ndim != 3 or y.shape[0] != self.n:
                    raise DimensionMismatch(f"output must have shape ({self.n}, T, {m.ny})")
                self._check_io(u.shape[2], y.shape[2], T, y.shape[1])
            else:
                self._check_io(u.shape[2], m.ny, T, T)
                y = np.empty((self.n, T, m.ny), dtype=np.float64)
            ub = np.ascontiguousarray(u)
            self.lib.check(self.lib.L.acme_batch_run(self.h, ub.ctypes.data, y.ctypes.data, T, ACME_MEM_HOST, None))
            self._hold(ub, y)
            if check:
                self.check()
            return y
        single = u.ndim == 2
        if single:
            if self.n != 1:
                raise DimensionMismatch("2-D input given to a runner with more than one instance")
            u = u[None]
        if u.ndim != 3 or u.shape[0] != self.n:
            raise DimensionMismatch(f"input must have shape ({self.n}, {m.nu}, T)")
        T = u.shape[2]
        if y is not None:
            y = np.asarray(y)
            yy = y[None] if single else y
            self._check_io(u.shape[1], yy.shape[1], T, yy.shape[2])
        else:
            self._check_io(u.shape[1], m.ny, T, T)
        ub = np.ascontiguousarray(np.transpose(u, (0, 2, 1)))        # [N][T][nu]
        yb = np.empty((self.n, T, m.ny), dtype=np.float64)
        self.lib.check(self.lib.L.acme_batch_run(
            self.h, ub.ctypes.data, yb.ctypes.data, T, ACME_MEM_HOST, None))
        self._hold(ub, yb)
        out = np.transpose(yb, (0, 2, 1))
        if y is not None:
            (y[None] if single else y)[...] = out
        if check:
            self.check()
        if y is not None:
            return y
        return np.asfortranarray(out[0]) if single else np.ascontiguousarray(out)

    def run_const(self, u_var, u_const, const_rows, y=None, check=True):
        """``run!`` with constant input rows (``acme_batch_run_const``): ``const_rows`` names the input rows that keep one
        value per instance for the whole call -- ``u_const`` (N, nu): their values (the other entries are ignored) --,
        ``u_var`` (N, T, nu_var) holds the remaining rows in row order (the ABI's time-major layout).  A sweep over
        potentiometer positions then moves a quarter of the bytes over the bus; the results are those of ``run`` on the
        materialised input, bit for bit.  Returns y (N, T, ny)."""
        m = self.model
        rows = sorted(set(int(k) for k in const_rows))
        if any(k < 0 or k >= m.nu for k in rows):
            raise DimensionMismatch(f"constant rows {rows} of a model with {m.nu} inputs")
        mask = 0
        for k in rows:
            mask |= 1 << k
        nuv = m.nu - len(rows)
        u_var = np.ascontiguousarray(u_var, dtype=np.float64)
        u_const = np.ascontiguousarray(u_const, dtype=np.float64)
        if u_var.ndim != 3 or u_var.shape[0] != self.n or u_var.shape[2] != nuv:
            raise DimensionMismatch(f"u_var must have shape ({self.n}, T, {nuv})")
        if u_const.shape != (self.n, m.nu):
            raise DimensionMismatch(f"u_const must have shape ({self.n}, {m.nu})")
        T = u_var.shape[1]
        if y is False:                  # (measure_const: no outputs)
            self.lib.check(self.lib.L.acme_batch_run_const(self.h, u_var.ctypes.data, u_const.ctypes.data, mask, None, T, ACME_MEM_HOST, None))
            self._hold(u_var, u_const)
            if check:
                self.check()
            return self
        if y is None:
            y = np.empty((self.n, T, m.ny), dtype=np.float64)
        elif not (isinstance(y, np.ndarray) and y.dtype == np.float64 and y.flags.c_contiguous and y.shape == (self.n, T, m.ny)):
            raise DimensionMismatch(f"y must be a C-contiguous float64 array of shape ({self.n}, {T}, {m.ny})")
        self.lib.check(self.lib.L.acme_batch_run_const(self.h, u_var.ctypes.data, u_const.ctypes.data, mask, y.ctypes.data, T, ACME_MEM_HOST, None))
        self._hold(u_var, u_const, y)
        if check:
            self.check()
        return y

    def run_async(self, u, y):
        """``acme_batch_run_async`` on host buffers in the ABI's layout: ``u`` (N, T, nu) and ``y``
        (N, T, ny), C-contiguous float64 (slices of larger arrays along the first axis are fine).
        Returns at once; ``wait()`` joins the run.  The caller keeps ``u`` / ``y`` alive until then.  ``y=None`` while a
        measurement is armed: the run only feeds the measurement."""
        m = self.model
        if y is None and self._meas is not None:
            if not (isinstance(u, np.ndarray) and u.dtype == np.float64 and u.flags.c_contiguous):
                raise TypeError("u must be a C-contiguous float64 array")
            if u.ndim != 3 or u.shape[0] != self.n or u.shape[2] != m.nu:
                raise DimensionMismatch(f"u must have shape ({self.n}, T, {m.nu})")
            self._inflight = (u,)
            self._hold(u)
            self.lib.check(self.lib.L.acme_batch_run_async(self.h, u.ctypes.data, None, u.shape[1], ACME_MEM_HOST, None))
            return
        for a, cols, what in ((u, m.nu, "u"), (y, m.ny, "y")):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
                raise TypeError(f"{what} must be a C-contiguous float64 array")
            if a.ndim != 3 or a.shape[0] != self.n or a.shape[2] != cols:
                raise DimensionMismatch(f"{what} must have shape ({self.n}, T, {cols})")
        self._check_io(u.shape[2], y.shape[2], u.shape[1], y.shape[1])
        self._inflight = (u, y)
        self._hold(u, y)
        self.lib.check(self.lib.L.acme_batch_run_async(self.h, u.ctypes.data, y.ctypes.data, u.shape[1],
                                                       ACME_MEM_HOST, None))

    def wait(self, check=True):
        """``acme_batch_wait``: join the run started by ``run_async``; raises what it failed with."""
        try:
            self.lib.check(self.lib.L.acme_batch_wait(self.h))
        finally:
            self._inflight = None
        if check:
            self.check()

    def run_device(self, u_ptr, y_ptr, T, stream=None):
        """Raw asynchronous launch: ``u_ptr``/``y_ptr`` are device addresses of
        [N][T][nu] / [N][T][ny] float64 buffers on this runner's GPU."""
        self.lib.check(self.lib.L.acme_batch_run(
            self.h, C.c_void_p(u_ptr), C.c_void_p(y_ptr), int(T), ACME_MEM_DEVICE,
            C.c_void_p(stream or 0)))

    def run_torch(self, u, y=None):
        """``u``: torch float64 CUDA tensor (N, T, nu); returns/fills ``y`` (N, T, ny).
        Launches on torch's current stream, does not synchronise."""
        import torch
        m = self.model
        if u.dtype != torch.float64 or not u.is_cuda or not u.is_contiguous():
            raise TypeError("u must be a contiguous float64 CUDA tensor")
        if u.dim() != 3 or u.shape[0] != self.n or u.shape[2] != m.nu:
            raise DimensionMismatch(f"u must have shape ({self.n}, T, {m.nu})")
        T = u.shape[1]
        if y is None:
            y = torch.empty((self.n, T, m.ny), dtype=torch.float64, device=u.device)
        elif tuple(y.shape) != (self.n, T, m.ny) or y.dtype != torch.float64 or not y.is_contiguous():
            raise DimensionMismatch(f"y must be a contiguous float64 tensor of shape ({self.n}, {T}, {m.ny})")
        stream = torch.cuda.current_stream(u.device).cuda_stream
        self.run_device(u.data_ptr(), y.data_ptr(), T, stream)
        return y

    # ---- reports, failure policy ----------------------------------------------------------
    def reports(self):
        r = (Report * self.n)()
        self.lib.check(self.lib.L.acme_batch_get_report(self.h, r))
        return r

    def report_arrays(self):
        r = self.reports()
        a = np.frombuffer(r, dtype=np.int64).reshape(self.n, 5).copy()
        return dict(n_warn=a[:, 0], first_nonconverged=a[:, 1], first_nonfinite=a[:, 2],
                    iters_total=a[:, 3], iters_max=a[:, 4])

    def check(self):
        """Apply step!'s policy (src/ACME.jl:688-694) to the accumulated reports."""
        ra = self.report_arrays()
        if (ra["first_nonfinite"] >= 0).any():
            i = int(np.argmax(ra["first_nonfinite"] >= 0))
            raise AcmeError("Failed to converge while solving non-linear equation, got non-finite "
                            f"result. (instance {i}, sample {int(ra['first_nonfinite'][i])})")
        nw = int(ra["n_warn"].sum())
        if nw > self._warned:
            warnings.warn("Failed to converge while solving non-linear equation.")
            self._warned = nw

    def reset_report(self):
        self.lib.check(self.lib.L.acme_batch_reset_report(self.h))
        self._warned = 0

    def last_kernel_ms(self):
        ms = C.c_float()
        self.lib.check(self.lib.L.acme_batch_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def kernel_time(self, reset=False):
        """(total ms, launches) of the kernels since the last reset, from HIP events."""
        ms, n = C.c_double(), C.c_longlong()
        self.lib.check(self.lib.L.acme_batch_kernel_time(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    # ---- solver plugin surface ----------------------------------------------------------------
    def set_resabstol(self, tol):
        """``set_resabstol!`` (src/solvers.jl:181,262)."""
        self.lib.check(self.lib.L.acme_batch_set_resabstol(self.h, float(tol)))

    def solve(self, p, sub=0):
        """Batched ``solve(model.solvers[sub+1], p)`` (src/solvers.jl:207-236, 268-302): ``p`` is
        (N, np); returns ``(z, hasconverged, needediterations)`` with shapes (N, nn), (N,), (N,).
        Uses and updates each instance's extrapolation origin like the reference's solver objects."""
        s = self.model.subs[sub]
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(p, dtype=np.float64), (self.n, s.np)))
        z = np.zeros((self.n, s.nn))
        conv = np.zeros(self.n, dtype=np.int32)
        iters = np.zeros(self.n, dtype=np.int32)
        self.lib.check(self.lib.L.acme_batch_solve(self.h, int(sub), _dp(p), _dp(z), _ip(conv), _ip(iters),
                                                   ACME_MEM_HOST, None))
        return z, conv.astype(bool), iters

    def get_extrapolation_jacobian(self, sub=0):
        """Batched ``get_extrapolation_jacobian(model.solvers[sub+1])`` (src/solvers.jl:198-201):
        (N, nn, np) array of dz/dp = -(J \\ Jp) at every instance's extrapolation origin."""
        s = self.model.subs[sub]
        jac = np.zeros((self.n, s.np, s.nn))          # ABI layout: per instance column-major nn x np
        self.lib.check(self.lib.L.acme_batch_get_extrapolation_jacobian(self.h, int(sub), _dp(jac), ACME_MEM_HOST, None))
        return np.ascontiguousarray(jac.transpose(0, 2, 1))

    def get_state(self):
        """(x, last_p, last_z): model.x and the extrapolation origin of every instance."""
        m = self.model
        x = np.zeros((self.n, m.nx))
        p = np.zeros((self.n, sum(s.np for s in m.subs)))
        z = np.zeros((self.n, sum(s.nn for s in m.subs)))
        self.lib.check(self.lib.L.acme_batch_get_state(self.h, _dp(x), _dp(p), _dp(z)))
        return x, p, z

    def set_state(self, x=None, p=None, z=None):
        def prep(a, cols):
            if a is None:
                return None, None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (self.n, cols)))
            return a, _dp(a)
        m = self.model
        xa, xp = prep(x, m.nx)
        pa, pp = prep(p, sum(s.np for s in m.subs))
        za, zp = prep(z, sum(s.nn for s in m.subs))
        self.lib.check(self.lib.L.acme_batch_set_state(self.h, xp, pp, zp))

    def kernel_shape(self):
        return self._mh.kernel_shape()

    def kernel_variant(self):
        return self._mh.kernel_variant()

    def kernel_family(self):
        """the kernel family THIS BATCH runs in ("tuned", "generic", "coop"): its model's, unless acme_batch_set_matrices moved
        it (instances with element parameters of their own)"""
        fam = C.c_int(0)
        self.lib.check(self.lib.L.acme_batch_kernel_variant(self.h, None, C.byref(fam)))
        return ("tuned", "generic", "coop")[fam.value]

    def batch_kernel_variant(self):
        """(condensed_rows, family) of the batch as it runs now (``acme_batch_kernel_variant``)"""
        nl, fam = C.c_int(0), C.c_int(0)
        self.lib.check(self.lib.L.acme_batch_kernel_variant(self.h, C.byref(nl), C.byref(fam)))
        return nl.value, ("tuned", "generic", "coop")[fam.value]


class MultiDeviceRunner:
    """N instances of a model spread over several GPUs of ONE node by ONE process: contiguous instance
    ranges (``dist.shard_range``), one ``ModelRunner`` per device, every run started asynchronously on all
    of them (``acme_batch_run_async``) and then joined, each batch reading and writing its own slice of
    the caller's ``u`` / ``y``.  No collective is involved -- the sweep shards perfectly -- so this is the
    multi-GPU path of a host that has no torch.distributed (the Julia binding's ``MultiBatchRunner`` is
    the same thing over the same C ABI).  ``devices``: HIP ordinals, default all visible ones; an ordinal
    may repeat (several batches on one GPU), which is how the path is tested on a single-GPU box."""

    def __init__(self, model, n_instances, devices=None, lib=None, models=None):
        from .dist import shard_range
        self.lib = lib or default_library()
        if devices is None:
            devices = list(range(self.lib.device_count()))
        if not devices:
            raise AcmeError("no HIP device available; acme_jl_amd has no CPU fallback")
        self.model, self.n, self.devices = model, int(n_instances), list(devices)
        self.ranges = [shard_range(self.n, k, len(self.devices)) for k in range(len(self.devices))]
        self.runners = []
        for dev, (lo, hi) in zip(self.devices, self.ranges):
            if hi > lo:
                part = None if models is None else [models[i] for i in range(lo, hi)]
                self.runners.append(ModelRunner(model, hi - lo, device=dev, lib=self.lib, models=part))
            else:
                self.runners.append(None)

    def set_oversampling(self, factor, up=None, down=None, held_rows=()):
        """``ModelRunner.set_oversampling`` on every device's batch"""
        for r in self.runners:
            if r is not None:
                r.set_oversampling(factor, up, down, held_rows)
        return self

    def set_measurement(self, start=0, length=0, f0=None, harmonics=0, rows=None, f_den=None, f_num=None, f0_from_source=None):
        """``ModelRunner.set_measurement`` on every device's batch, per-instance ``f_num`` sliced over the devices"""
        if f_num is not None and np.ndim(f_num) != 0 and len(f_num) != self.n:
            raise DimensionMismatch(f"per-instance fundamentals need {self.n} values")
        for r, (lo, hi) in zip(self.runners, self.ranges):
            if r is not None:
                part = f_num if f_num is None or np.ndim(f_num) == 0 else np.asarray(f_num)[lo:hi]
                r.set_measurement(start, length, f0, harmonics, rows, f_den, part, f0_from_source)
        return self

    def set_measurement_bins(self, coef, start=0, length=0, rows=None, f_den=None, f_num=None, tones_from_source=None):
        """``ModelRunner.set_measurement_bins`` on every device's batch, per-instance ``f_num`` (tones, N) sliced over the devices"""
        if f_num is not None and np.ndim(f_num) == 2 and np.shape(f_num)[1] not in (1, self.n):
            raise DimensionMismatch(f"per-instance tones need (tones, {self.n}) values")
        for r, (lo, hi) in zip(self.runners, self.ranges):
            if r is not None:
                part = f_num if f_num is None or np.ndim(f_num) < 2 or np.shape(f_num)[1] == 1 else np.asarray(f_num)[:, lo:hi]
                r.set_measurement_bins(coef, start, length, rows, f_den, part, tones_from_source)
        return self

    def reset_measurement(self):
        for r in self.runners:
            if r is not None:
                r.reset_measurement()
        return self

    def measurement(self):
        """the shards' ``Measurement`` results, concatenated along the instances"""
        return Measurement.concatenate([r.measurement() for r in self.runners if r is not None])

    def set_measurement_series(self, win, hop=None, windows=1):
        """``ModelRunner.set_measurement_series`` on every device's batch"""
        for r in self.runners:
            if r is not None:
                r.set_measurement_series(win, hop, windows)
        return self

    def measurement_series(self, first=0, n=None):
        """the shards' ``MeasurementSeries`` results, concatenated along the instances"""
        return MeasurementSeries.concatenate([r.measurement_series(first, n) for r in self.runners if r is not None])

    def set_measurement_fold(self, period=None, period_from_source=None):
        """``ModelRunner.set_measurement_fold`` on every device's batch, per-instance periods sliced over the devices"""
        if period is not None and np.ndim(period) != 0 and len(period) != self.n:
            raise DimensionMismatch(f"per-instance periods need {self.n} values")
        for r, (lo, hi) in zip(self.runners, self.ranges):
            if r is not None:
                r.set_measurement_fold(period if period is None or np.ndim(period) == 0 else np.asarray(period)[lo:hi],
                                       period_from_source)
        return self

    def measurement_fold(self, raw=False):
        """the shards' ``MeasurementFold`` results, concatenated along the instances (``raw`` as ``ModelRunner``'s)"""
        return MeasurementFold.concatenate([r.measurement_fold(raw) for r in self.runners if r is not None])

    def set_measurement_spectrum(self, nfft, hop=None, window="hann"):
        """``ModelRunner.set_measurement_spectrum`` on every device's batch"""
        for r in self.runners:
            if r is not None:
                r.set_measurement_spectrum(nfft, hop, window)
        return self

    def measurement_spectrum(self, raw=False):
        """the shards' ``MeasurementSpectrum`` results, concatenated along the instances (``raw`` as ``ModelRunner``'s)"""
        return MeasurementSpectrum.concatenate([r.measurement_spectrum(raw) for r in self.runners if r is not None])

    def set_measurement_cross(self, in_row, nfft, hop=None, window="hann"):
        """``ModelRunner.set_measurement_cross`` on every device's batch"""
        for r in self.runners:
            if r is not None:
                r.set_measurement_cross(in_row, nfft, hop, window)
        return self

    def measurement_cross(self, raw=False):
        """the shards' ``MeasurementCross`` results, concatenated along the instances (``raw`` as ``ModelRunner``'s)"""
        return MeasurementCross.concatenate([r.measurement_cross(raw) for r in self.runners if r is not None])

    def set_measurement_target(self, target, which=None, lag=None, preemphasis=0.0):
        """``ModelRunner.set_measurement_target`` on every device's batch, per-instance ``which`` and ``lag`` sliced over the
        devices (every batch holds the whole table)"""
        for a, what in ((which, "which"), (lag, "lag")):
            if a is not None and np.ndim(a) != 0 and len(a) != self.n:
                raise DimensionMismatch(f"per-instance {what} needs {self.n} values")
        part = lambda a, lo, hi: a if a is None or np.ndim(a) == 0 else np.asarray(a)[lo:hi]
        for r, (lo, hi) in zip(self.runners, self.ranges):
            if r is not None:
                r.set_measurement_target(target, part(which, lo, hi), part(lag, lo, hi), preemphasis)
        return self

    def measurement_target(self, raw=False):
        """the shards' ``MeasurementTarget`` results, concatenated along the instances (``raw`` as ``ModelRunner``'s)"""
        return MeasurementTarget.concatenate([r.measurement_target(raw) for r in self.runners if r is not None])

    def set_measurement_ensemble(self, groups=None, n_groups=None, stride=1):
        """``ModelRunner.set_measurement_ensemble`` on every device's batch, ``groups`` sliced over the devices.  Every group
        must lie wholly in one device's range of instances: a chain over shards would not be the chain over one device
        (``ValueError`` naming the group otherwise)."""
        ga = np.zeros(self.n, dtype=np.int64) if groups is None else np.asarray(groups)
        if ga.shape != (self.n,):
            raise DimensionMismatch(f"groups needs {self.n} values")
        G = int(n_groups) if n_groups is not None else max(int(ga.max(initial=-1)) + 1, 1)
        owner = {}
        for k, (lo, hi) in enumerate(self.ranges):
            for g in np.unique(ga[lo:hi]):
                if g >= 0 and owner.setdefault(int(g), k) != k:
                    raise ValueError(f"group {int(g)} has members on more than one device (shards {owner[int(g)]} and {k}): "
                                     "an ensemble's chains do not cross devices")
        for r, (lo, hi) in zip(self.runners, self.ranges):
            if r is not None:
                r.set_measurement_ensemble(ga[lo:hi], G, stride)
        return self

    def measurement_ensemble(self):
        """the shards' ``MeasurementEnsemble`` results joined by group, the indices those of the whole batch"""
        live = [(r, lo) for r, (lo, hi) in zip(self.runners, self.ranges) if r is not None]
        return MeasurementEnsemble.join([r.measurement_ensemble() for r, _ in live], [lo for _, lo in live])

    def set_measurement_histogram(self, bins, lo, hi, mode="signed"):
        """``ModelRunner.set_measurement_histogram`` on every device's batch, ``lo`` and ``hi`` (scalars or N values) sliced
        over the devices' instances"""
        for name, a in (("lo", lo), ("hi", hi)):
            if np.ndim(a) != 0 and np.shape(a) != (self.n,):
                raise DimensionMismatch(f"{name} needs {self.n} values (or a scalar)")
        part = lambda a, lo_, hi_: a if np.ndim(a) == 0 else np.asarray(a)[lo_:hi_]
        for r, (a, b) in zip(self.runners, self.ranges):
            if r is not None:
                r.set_measurement_histogram(bins, part(lo, a, b), part(hi, a, b), mode)
        return self

    def measurement_histogram(self):
        """the shards' ``MeasurementHistogram`` results, concatenated along the instances (nothing joins across shards)"""
        return MeasurementHistogram.concatenate([r.measurement_histogram() for r in self.runners if r is not None])

    def set_measurement_events(self, levels=None, hysteresis=0.0, slots=8, lo=None, hi=None):
        """``ModelRunner.set_measurement_events`` on every device's batch, (C, N) levels sliced over the devices' instances"""
        def part(a, lo_, hi_):
            if a is None or np.ndim(a) < 2:
                return a
            if np.shape(a)[1] not in (1, self.n):
                raise DimensionMismatch(f"the levels need C or (C, {self.n}) values")
            return a if np.shape(a)[1] == 1 else np.asarray(a)[:, lo_:hi_]
        for r, (a, b) in zip(self.runners, self.ranges):
            if r is not None:
                r.set_measurement_events(part(levels, a, b), hysteresis, slots, part(lo, a, b), part(hi, a, b))
        return self

    def measurement_events(self):
        """the shards' ``MeasurementEvents`` results, concatenated along the instances (nothing joins across shards)"""
        return MeasurementEvents.concatenate([r.measurement_events() for r in self.runners if r is not None])

    def set_measurement_weighting(self, sos):
        """``ModelRunner.set_measurement_weighting`` on every device's batch: the same cascade everywhere"""
        for r in self.runners:
            if r is not None:
                r.set_measurement_weighting(sos)
        return self

    def measurement_weighting(self):
        """the cascade the shards share: a ``MeasurementWeighting``"""
        return next(r for r in self.runners if r is not None).measurement_weighting()

    def measure(self, u=None, check=True, T=None):
        """``run`` with y = NULL on every device (``u``: (N, T, nu), the ABI's layout); only the measurements are fed.
        ``u=None`` when every input row has a source: ``T`` samples are generated on the devices."""
        if u is None:
            return self.run_sources(T, y=False, check=check)
        return self.run(u, y=False, check=check)

    # ---- sources: the per-instance parameters sliced over the devices ---------------------------
    def set_source(self, row, kind, amp=None, offset=None, f_den=None, f_num=None, phase=None, table=None,
                   dist="gaussian", hold=1, stream=None, seed=0, period=None, delay=None, rise=None, on=None, fall=None, at=None):
        """``ModelRunner.set_source`` on every device's batch, each with its instances' parameters (a noise source's
        streams are formed over the global instance index: a sharded batch renders what the single batch renders; a pulse's
        or burst's five integers are sliced as the other parameters are)"""
        multi = _SOURCE_KINDS.get(kind) == SOURCE_MULTISINE
        streams = noise_streams(self.n, stream, seed) if _SOURCE_KINDS.get(kind) == SOURCE_NOISE else None

        def part(a, lo, hi):
            if multi and a is not None and np.ndim(a) == 2 and a is not offset:
                return a if np.shape(a)[1] == 1 else np.asarray(a)[:, lo:hi]
            if multi and a is not offset:
                return a                    # ((tones,): one value per tone for every instance)
            return a if a is None or np.ndim(a) == 0 else np.asarray(a)[lo:hi]
        for a in (amp, offset, f_num, phase, period, delay, rise, on, fall, at):
            if multi and a is not offset:
                if a is not None and np.ndim(a) == 2 and np.shape(a)[1] not in (1, self.n):
                    raise DimensionMismatch(f"per-instance tone parameters need (tones, {self.n}) values")
            elif a is not None and np.ndim(a) != 0 and len(a) != self.n:
                raise DimensionMismatch(f"per-instance source parameters need {self.n} values")
        for r, (lo, hi) in zip(self.runners, self.ranges):
            if r is not None:
                r.set_source(row, kind, part(amp, lo, hi), part(offset, lo, hi), f_den, part(f_num, lo, hi), part(phase, lo, hi), table,
                             dist, hold, None if streams is None else streams[lo:hi], seed, part(period, lo, hi), part(delay, lo, hi),
                             part(rise, lo, hi), part(on, lo, hi), part(fall, lo, hi), part(at, lo, hi))
        return self

    def clear_source(self, row=-1):
        for r in self.runners:
            if r is not None:
                r.clear_source(row)
        return self

    @property
    def source_clock(self):
        return next(r for r in self.runners if r is not None).source_clock

    @source_clock.setter
    def source_clock(self, n):
        for r in self.runners:
            if r is not None:
                r.source_clock = n

    def run_sources(self, T=None, u_var=None, y=None, check=True):
        """``ModelRunner.run_sources`` on every device at once (``run_sources_async``, then joined): ``u_var`` (N, T, nu_var)
        or None, returns / fills ``y`` (N, T, ny); ``y=False``: no outputs (measurement armed), returns ``self``."""
        if u_var is not None:
            u_var = np.ascontiguousarray(u_var, dtype=np.float64)
            if u_var.ndim != 3 or u_var.shape[0] != self.n:
                raise DimensionMismatch(f"u_var must have shape ({self.n}, T, nu_var)")
            T = u_var.shape[1]
        if T is None:
            raise DimensionMismatch("every input row has a source: give the number of samples T")
        if y is None:
            y = np.empty((self.n, int(T), self.model.ny), dtype=np.float64)
        started, err = [], None
        for r, (lo, hi) in zip(self.runners, self.ranges):
            if r is not None:
                r.run_sources_async(T, None if u_var is None else u_var[lo:hi], None if y is False else y[lo:hi])
                started.append(r)
        for r in started:
            try:
                r.wait(check=check)
            except AcmeError as e:
                err = err or e
        if err is not None:
            raise err
        return self if y is False else y

    def render_sources(self, T=None, u_var=None):
        parts = [r.render_sources(T, None if u_var is None else np.asarray(u_var)[lo:hi])
                 for r, (lo, hi) in zip(self.runners, self.ranges) if r is not None]
        return np.concatenate(parts)

    def run(self, u, y=None, check=True):
        """``u``: (N, T, nu) C-contiguous float64 (the ABI's layout); returns / fills ``y`` (N, T, ny)."""
        m = self.model
        u = np.ascontiguousarray(u, dtype=np.float64)
        if y is False:                  # (measure: no outputs)
            if u.ndim != 3 or u.shape[0] != self.n or u.shape[2] != m.nu:
                raise DimensionMismatch(f"input must have shape ({self.n}, T, {m.nu})")
            started, err = [], None
            for r, (lo, hi) in zip(self.runners, self.ranges):
                if r is not None:
                    r.run_async(u[lo:hi], None)
                    started.append(r)
            for r in started:
                try:
                    r.wait(check=check)
                except AcmeError as e:
                    err = err or e
            if err is not None:
                raise err
            return self
        if u.ndim != 3 or u.shape[0] != self.n or u.shape[2] != m.nu:
            raise DimensionMismatch(f"input must have shape ({self.n}, T, {m.nu})")
        if y is None:
            y = np.empty((self.n, u.shape[1], m.ny), dtype=np.float64)
        elif y.shape != (self.n, u.shape[1], m.ny) or y.dtype != np.float64 or not y.flags.c_contiguous:
            raise DimensionMismatch(f"output must be a C-contiguous float64 array of shape ({self.n}, {u.shape[1]}, {m.ny})")
        started, err = [], None
        for r, (lo, hi) in zip(self.runners, self.ranges):
            if r is not None:
                r.run_async(u[lo:hi], y[lo:hi])
                started.append(r)
        for r in started:                       # join every run, then report the first failure
            try:
                r.wait(check=check)
            except AcmeError as e:
                err = err or e
        if err is not None:
            raise err
        return y

    def report_arrays(self):
        parts = [r.report_arrays() for r in self.runners if r is not None]
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}

    def get_state(self):
        parts = [r.get_state() for r in self.runners if r is not None]
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def run(model_or_runner, u, **kw):
    """``run!(model, u)`` / ``run!(runner, u)`` (src/ACME.jl:567-568, 619-623).  The model's
    state persists across calls: the runner is cached on the model object."""
    if isinstance(model_or_runner, ModelRunner):
        return model_or_runner.run(u, **kw)
    model = model_or_runner
    r = getattr(model, "_runner", None)
    if r is None:
        r = model._runner = ModelRunner(model, 1)
    return r.run(u, **kw)
