"""The measurement weighting (acme_batch_set_measurement_weighting) on the CPU wave emulator: a cascade of second-order
sections ahead of every measurement form, the weighted samples against a numpy replay of the contract on the stored y of an
identical run without a weighting, bit for bit, and every form on them through the existing replays (weighting_ref).

1. exact pins   2. geometry   3. every path   4. coexistence   5. life cycle, errors, a batch without a weighting is what it
was   6. a non-finite instance   7. use level: the K, A and C designs, scipy's layout, the loudness helper (CPU only)

The lengths, start and T are those of the GPU file.  The emulator walks the pairs one by one (partial waves and blocks do not
exist here), so the geometry runs at N = 3, the paths at N = 6 over T = 460 (the slices of 150 and the chunks of one tile are
what puts a slice's and a chunk's first sample at every phase of the cascade's states), the two-output model at N = 2 over
T = 1000.  test_gpu_measurement_weighting.py runs the full shapes, the loudness and target use cases and MultiDeviceRunner."""
import numpy as np
import pytest

import weighting_ref as WR

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")

_MK = {}


def mk_for(lib):
    """one maker per library, so that weighting_ref's shared plain runs are shared"""
    if id(lib) not in _MK:
        def mk(model, n, **kw):
            from acme_jl_amd.runner import ModelRunner
            return ModelRunner(model, n, lib=lib, **kw)
        _MK[id(lib)] = mk
    return _MK[id(lib)]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_identity_section_changes_nothing(emu_lib):
    WR.check_identity(mk_for(emu_lib), N=3, T=1500)


@pytest.mark.parametrize("case", ["delay", "delay, split", "1 2 1", "running sum", "8 delays"])
def test_exact_pins(emu_lib, case):
    WR.check_integer_pins(mk_for(emu_lib), case, N=3, T=1500)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S = 1", "S = 2", "S = 3", "S = 8", "A"])
def test_geometry(emu_lib, name):
    WR.check_geometry(mk_for(emu_lib), 3, 9000, 301, name)


@pytest.mark.parametrize("rows", [[1], None])
def test_two_outputs(emu_lib, rows):
    WR.check_geometry(mk_for(emu_lib), 2, 1000, 301, "S = 3", rows=rows, two=True)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
class HostDevice:
    """the emulator's "device memory" is host memory"""

    def put(self, a):
        return np.ascontiguousarray(a)

    def run(self, r, u, keep, T):
        from acme_jl_amd.runner import ModelRunner
        y = np.zeros((r.n, T, r.model.ny)) if keep else None
        ModelRunner.run_device(r, u.ctypes.data, y.ctypes.data if keep else 0, T)
        return y


@pytest.mark.parametrize("k", [1, 3])
def test_paths_are_bit_identical(emu_lib, monkeypatch, k):
    WR.check_paths(mk_for(emu_lib), HostDevice(), k, 460, monkeypatch, N=6)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_coexists_with_fold_spectrum_cross_and_target(emu_lib):
    WR.check_coexistence(mk_for(emu_lib), 5, 400)


def test_series_and_per_instance_harmonics_read_the_weighted_rows(emu_lib):
    WR.check_series_and_per_instance(mk_for(emu_lib), 3, 1300)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(emu_lib):
    WR.check_life_cycle(mk_for(emu_lib))


def test_set_matrices_carries_the_weighting(emu_lib):
    WR.check_set_matrices_carries_the_weighting(mk_for(emu_lib))


def test_argument_errors(emu_lib):
    WR.check_errors(mk_for(emu_lib))


def test_a_batch_without_a_weighting_is_unchanged(emu_lib):
    WR.check_no_weighting_invariance(mk_for(emu_lib), 67, 300)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_instance_reads_nan_only_itself(emu_lib):
    WR.check_nan_instance(mk_for(emu_lib))


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_k_weighting_is_the_table_of_bs1770():
    """(a) the formulas at 48 kHz against the standard's tables: 1e-12 (the deviation is 8.9e-16, rounding of the formulas)"""
    from acme_jl_amd.runner import weighting_sos
    k = weighting_sos("K", 48000)
    print("K at 48 kHz, deviation from the tables:", np.abs(k - WR.BS1770_48K).max())
    assert k.shape == (2, 5) and np.abs(k - WR.BS1770_48K).max() <= 1e-12


@pytest.mark.parametrize("fs", [44100, 48000])
@pytest.mark.parametrize("kind", ["A", "C"])
def test_a_and_c_are_the_bilinear_transform_of_the_analog_prototype(kind, fs):
    """(b) the bilinear identity H_d(e^{j 2 pi f / fs}) = H_a(j 2 fs tan(pi f / fs)), both scaled to 1 at 1 kHz: 1e-9 dB at
    31.5 Hz, 100 Hz, 1 kHz and 10 kHz (rounding only); |response(1000)| = 1 within 1e-12"""
    from acme_jl_amd.runner import MeasurementWeighting, weighting_sos
    sos = weighting_sos(kind, fs)
    assert sos.shape == ({"A": 3, "C": 2}[kind], 5)
    mw = MeasurementWeighting(sos)
    f = np.array([31.5, 100.0, 1000.0, 10000.0])
    warped = lambda f: 2.0 * fs * np.tan(np.pi * np.asarray(f) / fs) / (2.0 * np.pi)
    ha = WR.analog_weighting(kind, warped(f)) / abs(WR.analog_weighting(kind, warped(1000.0)))
    hd = mw.response(f, fs)
    db = 20.0 * np.log10(np.abs(hd / ha))
    print(kind, fs, "dB:", 20.0 * np.log10(np.abs(hd)), "deviation:", db, "phase:", np.angle(hd / ha))
    assert (np.abs(db) <= 1e-9).all() and (np.abs(np.angle(hd / ha)) <= 1e-9).all()
    assert abs(abs(mw.response(1000.0, fs)) - 1.0) <= 1e-12
    # what plain bilinear costs near Nyquist (the docstring's figures)
    if kind == "A" and fs == 44100:
        analog = 20.0 * np.log10(abs(WR.analog_weighting("A", 10000.0)) / abs(WR.analog_weighting("A", 1000.0)))
        assert round(float(20.0 * np.log10(abs(hd[3]))), 1) == -4.0 and round(float(analog), 1) == -2.5


def test_dc_blocker_and_kinds():
    from acme_jl_amd.runner import MeasurementWeighting, weighting_sos
    assert weighting_sos("dc", 48000, r=0.99).tolist() == [[1.0, -1.0, 0.0, -0.99, 0.0]]
    w = MeasurementWeighting(weighting_sos("dc", 48000)).apply(np.ones((2, 3000)))
    assert w.shape == (2, 3000) and w[0, 0] == 1.0 and abs(w[0, -1]) < 1e-6
    with pytest.raises(ValueError, match="kind"):
        weighting_sos("B", 48000)


def test_apply_is_the_replay_and_scipy_layout():
    from acme_jl_amd.runner import MeasurementWeighting, sos_rows
    sos = WR.stable_sos(8)
    x = np.random.default_rng(3).standard_normal((4, 2, 700))
    w = MeasurementWeighting(sos).apply(x)
    assert np.array_equal(w.transpose(0, 2, 1), WR.replay(np.ascontiguousarray(x.transpose(0, 2, 1)), sos))
    assert np.array_equal(MeasurementWeighting(sos).apply(x[1, 0]), w[1, 0])
    six = np.insert(sos, 3, 1.0, axis=1)
    assert np.array_equal(sos_rows(six), sos)
    six[2, 3] = 2.0
    with pytest.raises(ValueError, match="a0"):
        sos_rows(six)


def test_loudness_helper():
    from acme_jl_amd.runner import Measurement
    out = np.zeros((2, 1, 4))
    out[:, 0, 1] = [1.0, np.sqrt(0.5)]
    lk = Measurement(out, 10, (0,)).loudness()
    assert lk[0, 0] == -0.691 and abs(lk[1, 0] - (-0.691 + 10 * np.log10(0.5))) < 1e-12
