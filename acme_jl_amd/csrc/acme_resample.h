// acme_resample.h -- oversampled runs (acme_batch_set_oversampling): the model runs at k x the signal rate, u is
// interpolated to that rate and y decimated from it on the device, one time slice at a time (acme_api.inc run_os).
//
//   interpolation   s[m] = u[m / k] if k divides m, else 0;  u_os[m] = sum_{j < Lu} g[j] s[m - j],  g = k h_up
//                   held rows (mask): u_os[m] = u[floor(m / k)]
//   decimation      y[n] = sum_{j < Ld} h_down[j] y_os[n k + k - 1 - j]
//
// Every sum runs over ascending j as one chain of fma starting from 0: a result does not depend on where a slice
// boundary falls, on host or device memory, or on the backend's launch shape.  Per instance the library keeps the
// signals' past in a small HBM buffer ("history", time-major like u / y):
//   u   [N][Du][nu]      the Du = floor((Lu - 1) / k) base-rate samples before the slice
//   y   [N][Ld - 1][ny]  the Ld - 1 model-rate samples before the slice
// os_hist moves a slice's tail into it after the slice's reads (ordered on the launch stream); os_fill extends a
// signal's first sample into the past (the first run after the factor is set).
//
// One thread per (instance, base-rate sample): it produces the k model-rate samples of every input row (interpolation),
// or one output sample of every output row (decimation).  The taps are indexed by loop counters only -- wave-uniform
// loads --, each base-rate input sample is read once and feeds the k phases' accumulators in registers (the phase
// count is a template parameter: 2 ... 16).
//
// The per-element functions are host + device code; the launchers below are __global__ launches under hipcc and
// plain loops otherwise (the CPU emulator of tests/emu compiles acme_api.inc, and with it this file, with g++).
// The default lowpass (os_design) is host code: the one design the C ABI hands to Python and Julia.
#pragma once
#include <cmath>
#include <vector>

#include "acme_common.h"

namespace acme {

constexpr int OS_MAX_FACTOR = 16;
constexpr int OS_MAX_TAPS = 4096;

struct OsInterpArgs {
    const double *u;            // base-rate slice: instance i, sample t, row r at u[(i * pitch + t) * nu + r]
    double *hist;               // [n][du][nu]
    double *out;                // [n][k * len][nu], packed
    const double *g;            // lu taps (k h_up)
    long long n, len, pitch;
    int nu, lu, du;
    unsigned long long held;    // rows held (zero-order hold)
};

struct OsDecimArgs {
    const double *in;           // [n][k * len][ny], packed: the model-rate outputs of the slice
    const double *hist;         // [n][ld - 1][ny]
    double *y;                  // instance i, sample t, row r at y[(i * pitch + t) * ny + r]
    const double *h;            // ld taps
    long long n, len, pitch;
    int k, ny, ld;
};

// a signal's last `hl` samples before the next slice: [n][hl][rows] <- the slice's tail (src: instance i, sample t, row r at
// src[(i * pitch + t) * rows + r], len samples), or -- fill -- its first sample, repeated
struct OsHistArgs {
    double *hist;
    const double *src;
    long long n, len, pitch;
    int rows, hl;
};

template <int K> ACME_HD inline void os_interp(const OsInterpArgs &A, long long idx) {
    const long long i = idx / A.len, t = idx - i * A.len;
    const int nu = A.nu;
    const double *ui = A.u + i * A.pitch * nu;
    const double *hi = A.hist + i * (long long)A.du * nu;
    double *o = A.out + (i * A.len + t) * K * nu;
    for (int r = 0; r < nu; ++r) {
        if (r < 64 && (A.held >> r & 1ull)) {
            const double v = ui[t * nu + r];
            for (int p = 0; p < K; ++p) o[p * nu + r] = v;
            continue;
        }
        double acc[K];
        for (int p = 0; p < K; ++p) acc[p] = 0.0;
        // u_os[t k + p] = sum over q of g[p + k q] u[t - q]: input sample t - q feeds tap p + k q of every phase p
        for (int q = 0; q <= A.du; ++q) {
            const long long s = t - q;
            const double v = s >= 0 ? ui[s * nu + r] : hi[(A.du + s) * nu + r];
            for (int p = 0; p < K; ++p) {
                const int j = p + K * q;
                if (j < A.lu) acc[p] = fma(A.g[j], v, acc[p]);
            }
        }
        for (int p = 0; p < K; ++p) o[p * nu + r] = acc[p];
    }
}

ACME_HD inline void os_decim(const OsDecimArgs &A, long long idx) {
    const long long i = idx / A.len, t = idx - i * A.len;
    const int ny = A.ny, hl = A.ld - 1;
    const double *yi = A.in + i * A.len * A.k * ny;
    const double *hi = A.hist + i * (long long)hl * ny;
    for (int r = 0; r < ny; ++r) {
        double acc = 0.0;
        for (int j = 0; j < A.ld; ++j) {
            const long long m = t * A.k + A.k - 1 - j;          // >= k - ld >= -hl
            const double v = m >= 0 ? yi[m * ny + r] : hi[(hl + m) * ny + r];
            acc = fma(A.h[j], v, acc);
        }
        A.y[(i * A.pitch + t) * ny + r] = acc;
    }
}

// thread (i, r): in ascending d, so that a slice shorter than the history reads entries not yet moved
ACME_HD inline void os_hist(const OsHistArgs &A, long long idx) {
    const long long i = idx / A.rows;
    const int r = (int)(idx - i * A.rows);
    double *h = A.hist + i * (long long)A.hl * A.rows;
    const double *src = A.src + i * A.pitch * A.rows;
    for (int d = 0; d < A.hl; ++d) {
        const long long s = A.len - A.hl + d;
        h[d * A.rows + r] = s >= 0 ? src[s * A.rows + r] : h[(d + A.len) * A.rows + r];
    }
}

ACME_HD inline void os_fill(const OsHistArgs &A, long long idx) {
    const long long i = idx / A.rows;
    const int r = (int)(idx - i * A.rows);
    double *h = A.hist + i * (long long)A.hl * A.rows;
    const double v = A.src[i * A.pitch * A.rows + r];
    for (int d = 0; d < A.hl; ++d) h[d * A.rows + r] = v;
}

// ---- the library's default lowpass (host) ------------------------------------------------------------------------------
// Kaiser-windowed sinc at the model rate k fs: cut-off 0.45 fs (the middle of the transition band 0.40 ... 0.50 fs),
// designed for 90 dB (Kaiser's formulas: beta = 0.1102 (A - 8.7), length (A - 7.95) / (2.285 dw)) -- at least 80 dB from
// 0.50 fs, passband ripple below 1e-4 up to 0.40 fs.  Length L = m k + 1, odd: (L - 1) / k base-rate samples of delay for
// the pair.  Symmetric by construction, unit DC gain.  Factor 1: the single tap 1.
inline double os_bessel_i0(double x) {
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 500; ++k) {
        t *= (x / (2.0 * k)) * (x / (2.0 * k));
        s += t;
        if (t < 1e-17 * s) break;
    }
    return s;
}
inline std::vector<double> os_design(int k) {
    if (k <= 1) return {1.0};
    const double pi = 3.14159265358979323846, A = 90.0;
    const double dw = 2.0 * pi * 0.1 / k;
    int m = (int)std::ceil((A - 7.95) / (2.285 * dw) / k);
    if (k % 2 == 1 && m % 2 == 1) ++m;          // (odd length)
    const int L = m * k + 1;
    const double beta = 0.1102 * (A - 8.7), M = 0.5 * (L - 1), fc = 0.45 / k, w0 = os_bessel_i0(beta);
    std::vector<double> h((size_t)L);
    for (int i = 0; i < L; ++i) {
        const double x = i - M, r = 2.0 * i / (L - 1) - 1.0;
        const double s = x == 0.0 ? 2.0 * fc : std::sin(2.0 * pi * fc * x) / (pi * x);
        h[(size_t)i] = s * os_bessel_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / w0;
    }
    for (int i = 0; i < L / 2; ++i) h[(size_t)i] = h[(size_t)(L - 1 - i)] = 0.5 * (h[(size_t)i] + h[(size_t)(L - 1 - i)]);
    double sum = 0.0;
    for (double v : h) sum += v;
    for (double &v : h) v /= sum;
    return h;
}

}  // namespace acme

// ---- launchers ---------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
template <int K> __global__ __launch_bounds__(256) void acme_os_interp_kernel(acme::OsInterpArgs A) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < A.n * A.len) acme::os_interp<K>(A, idx);
}
__global__ __launch_bounds__(256) void acme_os_decim_kernel(acme::OsDecimArgs A) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < A.n * A.len) acme::os_decim(A, idx);
}
__global__ __launch_bounds__(256) void acme_os_hist_kernel(acme::OsHistArgs A, int fill) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= A.n * A.rows) return;
    if (fill) acme::os_fill(A, idx);
    else acme::os_hist(A, idx);
}
namespace acme {
using os_stream_t = hipStream_t;
inline unsigned os_grid(long long threads) { return (unsigned)((threads + 255) / 256); }
template <int K> inline int os_interp_k(const OsInterpArgs &A, os_stream_t st) {
    hipLaunchKernelGGL(acme_os_interp_kernel<K>, dim3(os_grid(A.n * A.len)), dim3(256), 0, st, A);
    return (int)hipGetLastError();
}
inline int os_launch_decim(const OsDecimArgs &A, os_stream_t st) {
    hipLaunchKernelGGL(acme_os_decim_kernel, dim3(os_grid(A.n * A.len)), dim3(256), 0, st, A);
    return (int)hipGetLastError();
}
inline int os_launch_hist(const OsHistArgs &A, bool fill, os_stream_t st) {
    hipLaunchKernelGGL(acme_os_hist_kernel, dim3(os_grid(A.n * A.rows)), dim3(256), 0, st, A, fill ? 1 : 0);
    return (int)hipGetLastError();
}
}  // namespace acme
#else
namespace acme {
using os_stream_t = void *;
template <int K> inline int os_interp_k(const OsInterpArgs &A, os_stream_t) {
    for (long long idx = 0; idx < A.n * A.len; ++idx) os_interp<K>(A, idx);
    return 0;
}
inline int os_launch_decim(const OsDecimArgs &A, os_stream_t) {
    for (long long idx = 0; idx < A.n * A.len; ++idx) os_decim(A, idx);
    return 0;
}
inline int os_launch_hist(const OsHistArgs &A, bool fill, os_stream_t) {
    for (long long idx = 0; idx < A.n * A.rows; ++idx) {
        if (fill) os_fill(A, idx);
        else os_hist(A, idx);
    }
    return 0;
}
}  // namespace acme
#endif

namespace acme {
inline int os_launch_interp(int k, const OsInterpArgs &A, os_stream_t st) {
    switch (k) {
    case 2: return os_interp_k<2>(A, st);
    case 3: return os_interp_k<3>(A, st);
    case 4: return os_interp_k<4>(A, st);
    case 5: return os_interp_k<5>(A, st);
    case 6: return os_interp_k<6>(A, st);
    case 7: return os_interp_k<7>(A, st);
    case 8: return os_interp_k<8>(A, st);
    case 9: return os_interp_k<9>(A, st);
    case 10: return os_interp_k<10>(A, st);
    case 11: return os_interp_k<11>(A, st);
    case 12: return os_interp_k<12>(A, st);
    case 13: return os_interp_k<13>(A, st);
    case 14: return os_interp_k<14>(A, st);
    case 15: return os_interp_k<15>(A, st);
    case 16: return os_interp_k<16>(A, st);
    default: return -1;
    }
}
}  // namespace acme
