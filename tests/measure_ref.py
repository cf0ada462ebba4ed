"""numpy form of the output measurements of include/acme_hip.h (acme_batch_set_measurement), shared by the emulator and
GPU tests."""
import numpy as np


def twiddles(f_num, f_den, H, m):
    """cos / sin [H, len(m)] of 2 pi ((h f_num m) mod f_den) / f_den, the phase reduced exactly in integers -- int64 and
    np.cos of the rounded angle, the library's own steps: it cannot disagree with meas_twiddle about the phase.  The
    independent form (unbounded integers, mpmath) is exact_ref.exact_twiddles."""
    h = np.arange(1, H + 1, dtype=np.int64)[:, None]
    k = (h * (f_num % f_den) % f_den) * (np.asarray(m, dtype=np.int64)[None] % f_den) % f_den
    k = np.where(2 * k > f_den, k - f_den, k)
    th = 2 * np.pi * (k / f_den)
    return np.cos(th), np.sin(th)


def np_measure(y, start=0, length=0, f0=(0, 1), H=0, rows=None):
    """y [N, T, ny]: the outputs of the T samples since arming -> (out [N, nrows, 4 + 2H], count), the layout of
    acme_batch_get_measurement"""
    N, T, ny = y.shape
    rows = list(range(ny)) if rows is None else list(rows)
    end = T if length == 0 else min(T, start + length)
    seg = y[:, start:end][:, :, rows]              # [N, n, nrows]
    n = max(end - start, 0)
    if n == 0:
        return None, 0
    out = np.empty((N, len(rows), 4 + 2 * H))
    out[:, :, 0] = seg.sum(axis=1) / n
    out[:, :, 1] = np.sqrt((seg ** 2).sum(axis=1) / n)
    out[:, :, 2] = seg.min(axis=1)
    out[:, :, 3] = seg.max(axis=1)
    if H:
        c, s = twiddles(f0[0], f0[1], H, np.arange(n))
        C_ = np.einsum("itr,ht->irh", seg, c)
        S_ = np.einsum("itr,ht->irh", seg, s)
        out[:, :, 4::2] = 2 * C_ / n
        out[:, :, 5::2] = -2 * S_ / n
    return out, n


def assert_measured(out, ref, rtol=1e-12):
    """every quantity within rtol of the row's RMS (min / max exactly)"""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    scale = np.maximum(ref[:, :, 1:2], 1e-300)
    err = np.abs(out - ref) / scale
    assert np.array_equal(out[:, :, 2:4], ref[:, :, 2:4])
    assert err.max() <= rtol, err.max()
