// acme_measure.h -- output measurements of a batch (acme_batch_set_measurement): per instance and measured output row the
// library accumulates, over the samples of a window, the sum, the sum of squares, min, max and for h = 1 ... H the two
// correlations of y with cos / sin of the h-th harmonic of the fundamental f = f_num / f_den x fs:
//
//   sum += y      sq = fma(y, y, sq)      min, max (NaN sticks)
//   C_h = fma(y, cos th, C_h)   S_h = fma(y, sin th, S_h)   th = 2 pi ((h f_num m) mod f_den) / f_den,  m = n - start
//
// Each accumulator is ONE chain in sample order, and the phase is reduced exactly in 64-bit integers (meas_twiddle, shared
// by host and device code): the result does not depend on where a slice or a call ends, on host or device memory, on the
// entry point or on whether y is stored.  The accumulators live in HBM, [4 + 2H][N nrows] (pair p = i nrows + j: instance
// i, j-th measured row), and carry from one slice to the next (acme_api.inc run_os: one step after the slice's run kernel
// or decimation).
//
// A step covers one chunk of at most MEAS_CHUNK samples: a small kernel writes the chunk's twiddles, [H][len] pairs
// (cos, sin) -- once per sample and harmonic, not per instance --, then the measurement kernel runs over the chunk.  Its
// block takes 64 pairs (a lane each) and one wave per UNIT: unit 0 the four moments, unit h the harmonic h; the H + 1
// units of a pair run side by side (grid.y splits them beyond 16 waves).  y is instance-major, so lanes that own
// instances would read 64 rows apart at every sample: the block stages tiles of 64 pairs x 64 samples through LDS with
// loads along the samples (contiguous per pair), and every wave then reads its lane's column.  A harmonic wave holds
// 64 samples' twiddles in its lanes and broadcasts the current one (v_readlane: no memory access).
//
// PER-INSTANCE FUNDAMENTALS (acme_batch_set_measurement_per_instance): instance i correlates with f_num[i] / f_den.  The
// instances are grouped by distinct f_num on the host at arming (meas_pi_plan): F groups, one table row [H][len] each, written
// by a twiddle kernel with a group index (meas_pi_tw: the same meas_twiddle per element).  The table is bounded:
// MEAS_PI_BUDGET = 64 MiB; the chunk length is the largest multiple of MEAS_TILE <= MEAS_CHUNK with F H len 16 B inside the
// budget, and one tile at least (every twiddle is a closed form of the sample's number and every accumulator one chain, so
// the chunk length cannot change a result).  Pairs go to lanes through a permutation sorted by group, and the rule between
// the two inner loops is:
//   a group's pairs fill whole waves (64 lanes) first, in group order; the remainders of all groups, again in group order,
//   share the waves behind them without padding.  A wave whose pairs share ONE group is UNIFORM and runs the broadcast
//   loop above on its group's table row; any other wave is MIXED: each lane reads its own group's (cos, sin) pairs with
//   16-byte loads, eight samples at a time ahead of the fma chain.
// Unit 0 (the moments) does not read the table: the same chain, the same bits.  F = 1 is the shared layout with one more
// indirection; F = N is mixed waves throughout with no idle lanes.
//
// BINS (acme_batch_set_measurement_bins): instance i has `tones` frequencies f_num[j][i] / f_den and bin b correlates with the
// integer combination k[b][i] = (sum_j coef[b][j] f_num[j][i]) mod f_den (the non-negative residue, formed on the host in
// exact 64-bit integers) -- the sum and difference products of a two-tone test.  The instances are grouped by distinct tone
// tuple, the table [F][B][len] is written from the groups' reduced bins kbin_g[F][B] (meas_bins_tw: meas_twiddle(1, m, k,
// f_den), the very twiddle of the shared form at f_num = k with one harmonic), and the plan, the budget, the chunk rule and
// acme_meas_pi_kernel with H = B are the per-instance form's, unchanged.
//
// SERIES (acme_batch_set_measurement_series): W windows of `win` samples, one every `hop` samples (1 <= win <= hop), all
// accumulated in the same pass.  With q = n - start the series-relative number of a sample, window w = q / hop holds it when
// m' = q - w hop < win; the samples of a gap (m' >= win) and those behind the last window belong to none.  Window w is, bit
// for bit, the single window [start + w hop, start + w hop + win): the twiddle is meas_twiddle(h, m', ...), every accumulator
// one chain in sample order from meas_init.  The accumulators are [W][4 + 2H][N nrows], slot w the layout above.  A chunk's
// table holds, at the chunk's sample t, the twiddle of that sample's m' (meas_series_tw; gap samples are neither written
// nor read), and ONE kernel per chunk (acme_meas_series_kernel<PI>: the block shape, the tiles and the plan of the kernels
// above) walks, tile by tile, the sub-ranges (window x tile) -- the same for every pair of the grid, hence wave-uniform: a
// window's first sample starts from meas_init in registers, a window that continues from an earlier chunk loads its slot,
// and the window's last sample -- or the chunk's -- stores the slot.  A tile that lies wholly in a gap is not staged.
//
// FOLD (acme_batch_set_measurement_fold): the window folded onto a period of P_i samples per instance, 1 <= P_i <=
// MEAS_MAX_FOLD_PERIOD -- slot s = m mod P_i of pair p accumulates fold[p][s] += y, ONE chain per slot, plain additions in
// sample order from 0.0.  The accumulators are [N nrows][Pmax], Pmax = max P_i.  One more kernel per chunk behind the
// measurement's own (acme_meas_fold_kernel), on the same chunk of y: ONE WAVE PER PAIR, so the period is wave-uniform and
// per-instance periods need no plan.  The phase ph = m0 mod P of the chunk's first sample is formed once per wave in 64-bit
// integers; lane l of block jb then owns the chunk's sample c = 64 jb + l < min(len, P) and with it the slot (ph + c) mod P,
// whose later samples follow at c + P, c + 2 P, ...: consecutive lanes read consecutive samples at every step (512
// contiguous bytes per wave instruction at ny = 1), every sample of the chunk is read once, a slot is loaded once and stored
// once, and a chunk shorter than the period touches the len slots it covers and no other.  Several blocks run side by side
// (independent chains: their loads are in flight together); a period below 64 leaves the lanes at and beyond P idle and
// takes several of a slot's samples ahead of its chain instead.
//
// SPECTRUM (acme_batch_set_measurement_spectrum): Welch-averaged periodograms of the window -- segment s covers the window's
// samples [s hop, s hop + L), L a power of two 64 ... 4096; x = w y, the radix-2 decimation-in-time transform with every
// operation rounded on its own (no fused multiply-add: include/acme_hip.h has the contract), acc[p][k] += Xr Xr + Xi Xi for
// k <= L / 2, ONE chain per bin in segment order from 0.0.  The accumulators are [N nrows][L / 2 + 1]; beside them a carry
// [N nrows][L], a ring per pair with window sample m at m mod L, holds the L most recent samples, so that a segment is
// transformed in the chunk that holds its last sample whatever chunks, slices and calls it straddles.  One more kernel per
// chunk (acme_meas_spectrum_kernel<log2 L>): a block of 256 lanes per pair, the vector in LDS, two stages a pass in
// registers; the emulator walks meas_spectrum_chain, the contract as a plain loop.
//
// CROSS-SPECTRUM (acme_batch_set_measurement_cross): the spectrum's segments of two real signals per pair -- x, one input row
// of the model as the run sees it at the base rate, and y, the measured row.  z = w x + i w y goes through ONE complex
// transform of the spectrum's (nothing assumed zero); X_k = (Z_k + conj Z_{L-k}) / 2 and Y_k = (Z_k - conj Z_{L-k}) / 2i are
// split off and four chains per bin accumulate |X|^2, |Y|^2 and the two parts of conj(X) Y in segment order from 0.0.  The
// accumulators are [N nrows][4][L / 2 + 1]; the carry is [N nrows][2][L], a ring of x and a ring of y per PAIR (a ring of x
// shared by an instance's rows would be rewritten by one row's block while another still reads it).  One more kernel per
// chunk (acme_meas_cross_kernel<log2 L>), the spectrum kernel's shape; the emulator walks meas_cross_chain.
//
// TARGET (acme_batch_set_measurement_target): the residual against a looped waveform of the caller's, t = tgt[which_i][j][(m +
// lag_i) mod P] -- seven chains per pair from 0.0, no fused multiply-add: See += (y - t)^2, Stt += t^2, Syt += y t, St += t,
// emax = max |y - t|, and behind the pre-emphasis 1 - c z^-1 Pee, Ptt; the two carries e_prev, t_prev live beside them.  The
// accumulators are [9][N nrows].  One more kernel per chunk (acme_meas_target_kernel): the moments unit's tiles, the chains
// of a pair split over three waves, a wave whose pairs share (which, row, lag) -- decided on the host at arming,
// meas_target_plan -- broadcasting its target tile, any other gathering per lane; the emulator walks meas_target_chain.
//
// WEIGHTING (acme_batch_set_measurement_weighting): a cascade of S <= 8 second-order sections, transposed direct form II, ahead
// of every form above -- per pair and sample, section after section, v = b0 x + s1, s1 = (b1 x - a1 v) + s2, s2 = b2 x - a2 v,
// x <- v, no fused multiply-add.  It runs on every base-rate output sample since arming; the states are [2 S][N nrows] (plane
// 2 k: s1 of section k, 2 k + 1: s2).  ONE kernel per slice (acme_meas_weight_kernel<S>) writes the weighted rows packed,
// [N][len][nrows], and every measurement kernel then reads that array with ny = nrows and the identity row table: the
// moments unit's tiles, four waves staging jointly through two LDS buffers, the next tile's loads in flight while the first
// wave walks the current tile's chains in place; the emulator walks meas_weight_chain.
//
// ENSEMBLE (acme_batch_set_measurement_ensemble): the one form that reduces over INSTANCES at one time sample -- the instances
// in G groups, window sample m recorded iff m mod stride == 0 in slot e = m / stride; per group, measured row and slot six
// values, each ONE chain over the group's members in ascending instance order, no fused multiply-add: S += v, Q += v v, the
// minimum and the maximum with the index of the member that set them (meas_min / meas_max with the index carried).  A slot
// is written exactly once, by the chunk that holds its sample; nothing carries.  The accumulators are plane-major,
// [6][G nrows][E] (S, Q, min, max as doubles, imin, imax as long long).  The plan -- the members sorted by (group, instance)
// and the groups' offsets [G + 1] -- is built on the host at arming.  One more kernel per chunk
// (acme_meas_ensemble_kernel<SPLIT>): a lane per recorded slot of the chunk, walking its group's member list with sixteen
// members' loads in flight ahead of the chains (at ny = 1, stride = 1 a wave's load is one member's 64 consecutive samples,
// 512 contiguous bytes); a block is four waves -- four tiles of 64 slots with all chains each, or, where that leaves fewer
// waves than the device has SIMDs, ONE tile with the four chains (S | Q | min | max) split over the waves; the emulator walks
// meas_ensemble_chain.
//
// HISTOGRAM (acme_batch_set_measurement_histogram): the amplitude distribution of every pair -- the one accumulator whose
// ADDRESS depends on the data.  Per sample exactly one of B + 3 integer counters of the pair goes up (meas_hist_bin: NAN,
// UNDER, OVER or bin k = trunc((x - lo_i) s_i) clamped to B - 1, the difference and the product rounded on their own, the
// scale s_i = B / (hi_i - lo_i) formed once on the host).  Counters are [n nrows][B + 3] long long in the result's order, the
// ranges [n][3].  One more kernel per chunk (acme_meas_hist_kernel<AGG>): one wave per pair, LDS atomic adds into the wave's
// own 32-bit counters, runs of equal counters among neighbouring lanes aggregated first, then a plain add of the non-zero
// ones into global memory; the pairs of a block follow from B (meas_hist_waves); the emulator walks meas_hist_chain.
//
// EVENTS (acme_batch_set_measurement_events): the one form that says WHEN -- per (instance, row, level) a state UNKNOWN / LOW /
// HIGH that v >= hi and v <= lo move (a comparator at lo == hi, a Schmitt trigger at lo < hi), five integer counters (RISE,
// FALL and the samples after which the state is HIGH, LOW, UNKNOWN), the first E events of either direction and the last one
// as (m, v[m - 1], v[m]), the values copied, and the state and the last value carried from chunk to chunk.  Comparisons and
// integers only: the host forms the sub-sample times.  One more kernel per chunk (acme_meas_events_kernel): one wave per pair,
// rounds of 64 consecutive samples, two ballots per level and round and the 64-bit mask algebra of meas_events_masks, which
// the non-HIP backend's mask walk shares; the emulator walks meas_events_chain, the contract's loop.
//
// The per-element functions are host + device code; the launchers below are __global__ launches under hipcc and plain
// loops otherwise (the CPU emulator of tests/emu compiles acme_api.inc, and with it this file, with g++).
#pragma once
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <vector>

#include "acme_common.h"

namespace acme {

constexpr int MEAS_MAX_H = 32;
constexpr long long MEAS_CHUNK = 4096;      // samples per measurement step (twiddle table: H x 4096 x 16 B at most)
constexpr int MEAS_TILE = 64;               // samples per LDS tile
constexpr int MEAS_MAX_WAVES = 16;          // waves (units) per block

struct MeasArgs {
    const double *y;            // instance i, sample t, row r at y[(i * pitch + t0 + t) * ny + r]
    double *acc;                // [4 + 2H][n * nrows]
    const double *tw;           // [H][len] pairs (cos, sin)
    long long n, len, pitch, t0;
    int ny, nrows, H;
    unsigned char row[64];      // the measured rows, ascending
};

struct MeasTwArgs {
    double *tw;                 // [H][len] pairs (cos, sin) of samples m0 ... m0 + len - 1 (window-relative)
    long long m0, len, f_num, f_den;    // 0 <= f_num < f_den < 2^31
    int H;
};

// per-instance fundamentals: the plan's device arrays beside the shared arguments (A.tw: [F][H][len] pairs)
struct MeasPiArgs {
    MeasArgs A;
    const long long *perm;      // [P]: slot -> pair, sorted by group as the rule above says
    const int *sgrp;            // [P]: slot -> group of its pair's instance
    const int *wgrp;            // [(P + 63) / 64]: wave -> its one group, or -1 (mixed)
};

struct MeasPiTwArgs {
    double *tw;                 // [F][H][len] pairs (cos, sin) of samples m0 ... m0 + len - 1 (window-relative)
    const long long *fnum_g;    // [F]: the groups' f_num, 0 <= f_num < f_den
    long long m0, len, f_den;
    int H, F;
};

// bins: the groups' reduced bin frequencies beside the table (A.tw: [F][B][len] pairs)
struct MeasBinsTwArgs {
    double *tw;                 // [F][B][len] pairs (cos, sin) of samples m0 ... m0 + len - 1 (window-relative)
    const long long *kbin_g;    // [F][B]: 0 <= k < f_den
    long long m0, len, f_den;
    int B, F;
};

constexpr long long MEAS_PI_BUDGET = 64ll << 20;    // bytes of twiddle table a chunk may take (one tile is always allowed)

// cos / sin of 2 pi ((h f_num m) mod f_den) / f_den, the phase reduced exactly (h <= 32, f_den < 2^31: products < 2^62)
// and taken to (-pi, pi] before the one rounding of the angle
// the angle 2 pi k / f_den of a reduced phase 0 <= k < f_den < 2^31, taken to (-pi, pi] first: two roundings, the quotient's
// and the product's (shared with the sine sources of acme_source.h)
ACME_HD inline double phase_angle(long long k, long long f_den) {
    if (2 * k > f_den) k -= f_den;
    return 6.283185307179586476925286766559 * ((double)k / (double)f_den);
}

ACME_HD inline void meas_twiddle(long long h, long long m, long long f_num, long long f_den, double *c, double *s) {
    const long long a = (h * f_num) % f_den;
    const long long k = (a * (m % f_den)) % f_den;
    const double th = phase_angle(k, f_den);
    *c = cos(th);
    *s = sin(th);
}

ACME_HD inline void meas_tw(const MeasTwArgs &A, long long idx) {
    const long long h = idx / A.len, t = idx - h * A.len;
    meas_twiddle(h + 1, A.m0 + t, A.f_num, A.f_den, &A.tw[2 * idx], &A.tw[2 * idx + 1]);
}

ACME_HD inline void meas_pi_tw(const MeasPiTwArgs &A, long long idx) {
    const long long per = A.H * A.len, g = idx / per, r = idx - g * per;
    const long long h = r / A.len, t = r - h * A.len;
    meas_twiddle(h + 1, A.m0 + t, A.fnum_g[g], A.f_den, &A.tw[2 * idx], &A.tw[2 * idx + 1]);
}

ACME_HD inline void meas_bins_tw(const MeasBinsTwArgs &A, long long idx) {
    const long long per = A.B * A.len, g = idx / per, r = idx - g * per;
    const long long b = r / A.len, t = r - b * A.len;
    meas_twiddle(1, A.m0 + t, A.kbin_g[g * A.B + b], A.f_den, &A.tw[2 * idx], &A.tw[2 * idx + 1]);
}

// series: the chunk's first sample is number s0 >= 0 of the series (n - start); the chunk lies inside the series' span
struct MeasSeries {
    long long win, hop, W, s0;
};

// the series' table of one chunk, for any of the three forms: [F][H][len] pairs, at sample t the twiddle of m' (F = 1 and
// fg = NULL: the shared form at f_num; bins: fg = kbin_g [F][H], every bin harmonic 1 of its reduced frequency)
struct MeasSeriesTwArgs {
    double *tw;
    const long long *fg;        // per-instance: [F] f_num; bins: [F][H] reduced bins; shared: NULL
    long long f_num, f_den, len;
    MeasSeries S;
    int H, F, bins;
};

struct MeasSeriesArgs {
    MeasPiArgs B;               // (the shared form: the plan's pointers NULL)
    MeasSeries S;
};

// window and window-relative number of the series' sample q, in exact 64-bit integers; false: q belongs to no window
ACME_HD inline bool meas_series_at(const MeasSeries &S, long long q, long long *w, long long *m) {
    *w = q / S.hop;
    *m = q - *w * S.hop;
    return *w < S.W && *m < S.win;
}

ACME_HD inline void meas_series_tw(const MeasSeriesTwArgs &A, long long idx) {
    const long long per = A.H * A.len, g = idx / per, r = idx - g * per;
    const long long h = r / A.len, t = r - h * A.len;
    long long w, m;
    if (!meas_series_at(A.S, A.S.s0 + t, &w, &m)) return;
    if (A.bins) meas_twiddle(1, m, A.fg[g * A.H + h], A.f_den, &A.tw[2 * idx], &A.tw[2 * idx + 1]);
    else meas_twiddle(h + 1, m, A.fg ? A.fg[g] : A.f_num, A.f_den, &A.tw[2 * idx], &A.tw[2 * idx + 1]);
}

// fold: the chunk's first sample is number m0 >= 0 of the window (n - start)
constexpr long long MEAS_MAX_FOLD_PERIOD = 65536;
constexpr int MEAS_FOLD_WAVES = 4;          // pairs (one wave each) per block

struct MeasFoldArgs {
    const double *y;            // instance i, sample t, row r at y[(i * pitch + t0 + t) * ny + r]
    double *fold;               // [n * nrows][pmax]
    const long long *per;       // [n]: the instances' periods, 1 <= per[i] <= pmax
    long long n, len, pitch, t0, m0, pmax;
    int ny, nrows;
    unsigned char row[64];      // the measured rows, ascending
};

// one pair over the chunk, sample after sample into the sample's slot (the reference order every backend keeps)
ACME_HD inline void meas_fold_chain(const MeasFoldArgs &A, long long p) {
    const long long i = p / A.nrows, P = A.per[i];
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    double *f = A.fold + p * A.pmax;
    long long s = A.m0 % P;
    for (long long t = 0; t < A.len; ++t) {
        f[s] += yp[t * A.ny];
        if (++s == P) s = 0;
    }
}

// spectrum: Welch-averaged periodograms of the window.  The chunk's first sample is number m0 >= 0 of the window; segment s
// covers the window's samples [s hop, s hop + L) and is transformed in the chunk that holds its last sample.  The samples
// of earlier chunks come from the carry, a ring per pair: sample m sits at carry[m mod L] (the L most recent samples).
constexpr long long MEAS_MIN_SPECTRUM = 64, MEAS_MAX_SPECTRUM = 4096;

struct MeasSpecArgs {
    const double *y;            // instance i, sample t, row r at y[(i * pitch + t0 + t) * ny + r]
    double *acc;                // [n * nrows][L / 2 + 1] sums of |X_k|^2, from 0.0
    double *carry;              // [n * nrows][L]
    const double *w;            // [L] the window
    const double *tw;           // [L / 2] pairs: (cos, -sin)(2 pi k / L)
    long long n, len, pitch, t0, m0, L, hop;
    int ny, nrows;
    unsigned char row[64];      // the measured rows, ascending
};

// the segments whose last sample lies in the chunk [m0, m0 + len): *lo ... *hi (none: *hi < *lo)
ACME_HD inline void meas_spec_segments(long long m0, long long len, long long L, long long hop, long long *lo, long long *hi) {
    *lo = m0 >= L ? (m0 - L + hop) / hop : 0;           // s hop + L - 1 >= m0
    *hi = m0 + len >= L ? (m0 + len - L) / hop : -1;    // s hop + L - 1 < m0 + len
}

// cross-spectrum: the spectrum's segments of TWO real signals per pair, x = input row in_row as the run sees it at the base
// rate and y = the measured row, packed into one complex transform.  S is the spectrum's argument block with
// acc [n * nrows][4][L / 2 + 1] (the planes xx, yy, re, im, from 0.0) and carry [n * nrows][2][L] (the ring of x, then the
// ring of y: sample m at m mod L)
struct MeasCrossArgs {
    MeasSpecArgs S;
    const double *u;            // instance i, sample t of the chunk at u[(i * upitch + t0 + t) * nu + in_row]
    long long upitch;
    int nu, in_row;
};

// Every operation of the spectrum is rounded on its own: no fused multiply-add (the compilers contract by default)
#if defined(__clang__)
#define ACME_NO_CONTRACT _Pragma("clang fp contract(off)")
#define ACME_NO_CONTRACT_FN
#else
#define ACME_NO_CONTRACT
#define ACME_NO_CONTRACT_FN __attribute__((optimize("fp-contract=off"), noinline))
#endif

// NaN sticks: once an accumulator is NaN it stays so
ACME_HD inline double meas_min(double m, double v) { return (v < m || v != v) ? v : m; }
ACME_HD inline double meas_max(double m, double v) { return (v > m || v != v) ? v : m; }

// the accumulators' start values: sum, sq 0; min +inf; max -inf; C_h, S_h 0
inline double meas_init(int a) { return a == 2 ? INFINITY : a == 3 ? -INFINITY : 0.0; }

// target: the chunk's first sample is number m0 >= 0 of the window (n - start).  acc is [MEAS_TARGET_SLOTS][n * nrows], the
// planes See, Stt, Syt, St, emax, Pee, Ptt and the two carries e_prev, t_prev, all from 0.0
constexpr int MEAS_MAX_TARGETS = 64;
constexpr int MEAS_TARGET_SLOTS = 9;
constexpr int MEAS_TARGET_WAVES = 3;        // the chains of a pair split over the waves of a block (acme_meas_target_kernel)

struct MeasTargetArgs {
    const double *y;            // instance i, sample t, row r at y[(i * pitch + t0 + t) * ny + r]
    double *acc;                // [MEAS_TARGET_SLOTS][n * nrows]
    const double *tgt;          // [K][nrows][P]
    const int *which;           // [n]: 0 <= which[i] < K
    const long long *lag;       // [n]: 0 <= lag[i] < P
    const int *wuni;            // [(n * nrows + 63) / 64]: != 0 -- the wave's pairs share (which, row, lag)
    long long n, len, pitch, t0, m0, P;
    double c;                   // the pre-emphasis coefficient
    int ny, nrows;
    unsigned char row[64];      // the measured rows, ascending
};

// one pair over the chunk, sample after sample: the contract of include/acme_hip.h as a plain loop (the reference order every
// backend keeps; every product and every sum rounded on its own)
ACME_HD ACME_NO_CONTRACT_FN inline void meas_target_chain(const MeasTargetArgs &A, long long p) {
    ACME_NO_CONTRACT
    const long long Pn = A.n * A.nrows, i = p / A.nrows, j = p - i * A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[j];
    const double *tg = A.tgt + ((long long)A.which[i] * A.nrows + j) * A.P;
    double *a = A.acc + p;
    double see = 0.0, stt = 0.0, syt = 0.0, st = 0.0, emax = 0.0, pee = 0.0, ptt = 0.0, ep = 0.0, tp = 0.0;
    if (A.m0 != 0) {            // (the window's first sample starts from 0.0 without reading)
        see = a[0]; stt = a[Pn]; syt = a[2 * Pn]; st = a[3 * Pn]; emax = a[4 * Pn]; pee = a[5 * Pn]; ptt = a[6 * Pn];
        ep = a[7 * Pn]; tp = a[8 * Pn];
    }
    long long s = (A.m0 % A.P + A.lag[i]) % A.P;
    for (long long k = 0; k < A.len; ++k) {
        const double y = yp[k * A.ny], t = tg[s];
        if (++s == A.P) s = 0;
        const double e = y - t;
        const double ee = e * e, tt = t * t, yt = y * t;
        see = see + ee;
        stt = stt + tt;
        syt = syt + yt;
        st = st + t;
        emax = meas_max(emax, fabs(e));
        const double ce = A.c * ep, ct = A.c * tp;
        const double de = e - ce, dt = t - ct;
        const double dee = de * de, dtt = dt * dt;
        pee = pee + dee;
        ptt = ptt + dtt;
        ep = e;
        tp = t;
    }
    a[0] = see; a[Pn] = stt; a[2 * Pn] = syt; a[3 * Pn] = st; a[4 * Pn] = emax; a[5 * Pn] = pee; a[6 * Pn] = ptt;
    a[7 * Pn] = ep; a[8 * Pn] = tp;
}

// the target's plan: per wave of 64 pairs whether they share (which, row, lag) -- then the wave takes its target tile once
template <class VI>
inline void meas_target_plan(const int *which, const long long *lag, long long n, int nrows, VI *wuni) {
    const long long Pn = n * nrows;
    wuni->assign((size_t)((Pn + 63) / 64), 0);
    for (long long w = 0; w * 64 < Pn; ++w) {
        const long long i0 = w * 64 / nrows, j0 = w * 64 - i0 * nrows;
        int u = 1;
        for (long long q = w * 64; q < Pn && q < w * 64 + 64; ++q) {
            const long long i = q / nrows;
            if (q - i * nrows != j0 || which[i] != which[i0] || lag[i] != lag[i0]) u = 0;
        }
        (*wuni)[(size_t)w] = u;
    }
}

// ensemble: the chunk's first sample is number m0 >= 0 of the window; window sample m is recorded iff m mod stride == 0, in
// slot e = m / stride.  acc is [4][G * nrows][E], the planes S, Q, min, max; arg is [2][G * nrows][E], the planes imin, imax
constexpr long long MEAS_MAX_ENSEMBLE = 1ll << 24;  // G nrows E at most (the table cap of the sources and the target)
constexpr int MEAS_ENS_WAVES = 4;           // waves per block: four tiles of slots, or one tile with the chains split (SPLIT)
constexpr int MEAS_ENS_AHEAD = 16;          // members whose loads are in flight ahead of the chains
constexpr long long MEAS_ENS_SPLIT_BELOW = 1024;    // SPLIT where the unsplit launch has fewer waves (256 CUs x 4 SIMDs)

struct MeasEnsArgs {
    const double *y;            // instance i, sample t, row r at y[(i * pitch + t0 + t) * ny + r]
    double *acc;                // [4][G * nrows][E]
    long long *arg;             // [2][G * nrows][E]
    const int *member;          // the instances that are in a group, sorted by (group, instance)
    const long long *off;       // [G + 1]: group g's members are member[off[g]] ... member[off[g + 1] - 1]
    long long len, pitch, t0, m0, stride, E;
    long long e0, nrec;         // the chunk's recorded slots e0 ... e0 + nrec - 1 (meas_ensemble_range)
    int G, ny, nrows;
    unsigned char row[64];      // the measured rows, ascending
};

// the slots whose samples lie in the chunk [m0, m0 + len): e0 = ceil(m0 / stride), and as many as fit
ACME_HD inline void meas_ensemble_range(long long m0, long long len, long long stride, long long *e0, long long *nrec) {
    *e0 = (m0 + stride - 1) / stride;
    const long long last = (m0 + len - 1) / stride;         // (len >= 1)
    *nrec = last >= *e0 ? last - *e0 + 1 : 0;
}

// the four chains' steps, shared by every backend: each rounded on its own, the extremes with the member's index carried
ACME_HD ACME_NO_CONTRACT_FN inline void meas_ens_sum(double &S, double v) {
    ACME_NO_CONTRACT
    S = S + v;
}
ACME_HD ACME_NO_CONTRACT_FN inline void meas_ens_sq(double &Q, double v) {
    ACME_NO_CONTRACT
    const double q = v * v;
    Q = Q + q;
}
ACME_HD inline void meas_ens_min(double &mn, long long &imin, double v, long long i) {
    if (v < mn || v != v) { mn = v; imin = i; }
}
ACME_HD inline void meas_ens_max(double &mx, long long &imax, double v, long long i) {
    if (v > mx || v != v) { mx = v; imax = i; }
}

// one (group, row) pair gr = g * nrows + j and one recorded slot e of the chunk, member after member: the contract of
// include/acme_hip.h as a plain loop (the reference order every backend keeps)
ACME_HD inline void meas_ensemble_chain(const MeasEnsArgs &A, long long gr, long long e) {
    const long long GR = (long long)A.G * A.nrows, g = gr / A.nrows, j = gr - g * A.nrows;
    const double *yp = A.y + (A.t0 + (e * A.stride - A.m0)) * A.ny + A.row[j];
    double S = 0.0, Q = 0.0, mn = INFINITY, mx = -INFINITY;
    long long imin = -1, imax = -1;
    for (long long k = A.off[g]; k < A.off[g + 1]; ++k) {
        const long long i = A.member[k];
        const double v = yp[i * A.pitch * A.ny];
        meas_ens_sum(S, v);
        meas_ens_sq(Q, v);
        meas_ens_min(mn, imin, v, i);
        meas_ens_max(mx, imax, v, i);
    }
    const long long at = gr * A.E + e, plane = GR * A.E;
    A.acc[at] = S; A.acc[plane + at] = Q; A.acc[2 * plane + at] = mn; A.acc[3 * plane + at] = mx;
    A.arg[at] = imin; A.arg[plane + at] = imax;
}

// the start values of one element of the planes: S, Q 0.0; min +inf; max -inf; imin, imax -1
ACME_HD inline void meas_ens_start(double *acc, long long *arg, long long plane, long long at) {
    acc[at] = 0.0; acc[plane + at] = 0.0; acc[2 * plane + at] = INFINITY; acc[3 * plane + at] = -INFINITY;
    arg[at] = -1; arg[plane + at] = -1;
}

// the ensemble's plan: the members sorted by (group, instance) and the groups' offsets; group NULL: all in group 0
template <class VI, class VL>
inline void meas_ensemble_plan(const int *group, long long n, int G, VI *member, VL *off) {
    off->assign((size_t)G + 1, 0);
    for (long long i = 0; i < n; ++i) {
        const int g = group ? group[i] : 0;
        if (g >= 0) ++(*off)[(size_t)g + 1];
    }
    for (int g = 0; g < G; ++g) (*off)[(size_t)g + 1] += (*off)[(size_t)g];
    member->assign((size_t)(*off)[(size_t)G], 0);
    std::vector<long long> at(off->begin(), off->end() - 1);
    for (long long i = 0; i < n; ++i) {     // (ascending i: every group's members in ascending instance order)
        const int g = group ? group[i] : 0;
        if (g >= 0) (*member)[(size_t)at[(size_t)g]++] = (int)i;
    }
}

// histogram: every sample of the chunk raises ONE of the B + 3 counters of its (instance, row) pair; cnt is
// [n * nrows][B + 3] in the result's order (UNDER, BIN[0 ... B - 1], OVER, NAN), range [n][3] = lo_i, hi_i, s_i
constexpr int MEAS_HIST_SIGNED = 0, MEAS_HIST_ABS = 1;
constexpr int MEAS_MAX_HIST_BINS = 4096;
constexpr long long MEAS_MAX_HISTOGRAM = 1ll << 28;     // N nrows (B + 3) counters at most (2 GiB of them)
constexpr int MEAS_HIST_WAVES = 4;          // pairs (one wave each) per block at most ...
constexpr int MEAS_HIST_LDS = 32768;        // ... and as many as keep a block's counters within these bytes of LDS
constexpr int MEAS_HIST_AHEAD = 8;          // loads a lane has in flight

struct MeasHistArgs {
    const double *y;            // instance i, sample t, row r at y[(i * pitch + t0 + t) * ny + r]
    long long *cnt;             // [n * nrows][B + 3]
    const double *range;        // [n][3]: lo, hi, s
    long long n, len, pitch, t0;
    int B, mode, ny, nrows;
    unsigned char row[64];      // the measured rows, ascending
};

// the scale, formed once at arming with two roundings: d = hi - lo; s = B / d
ACME_HD ACME_NO_CONTRACT_FN inline void meas_hist_scale(double lo, double hi, int B, double *d, double *s) {
    ACME_NO_CONTRACT
    *d = hi - lo;
    *s = (double)B / *d;
}

// the counter 0 ... B + 2 of one sample (x = v, or |v| in the ABS mode): the contract of include/acme_hip.h, the difference
// and the product rounded on their own
ACME_HD ACME_NO_CONTRACT_FN inline int meas_hist_bin(double x, double lo, double hi, double s, int B) {
    ACME_NO_CONTRACT
    if (x != x) return B + 2;
    if (x < lo) return 0;
    if (x >= hi) return B + 1;
    const double t = x - lo;
    const double q = t * s;
    long long k = (long long)q;         // truncation; q >= 0 here (-0.0 at lo = 0 included)
    if (k > B - 1) k = B - 1;           // q can round up to B just below hi
    return (int)k + 1;
}

// one pair over the chunk, sample after sample (the plain loop of the non-HIP backend; counters are integers, any order
// gives the same result)
ACME_HD inline void meas_hist_chain(const MeasHistArgs &A, long long p) {
    const long long i = p / A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    const double lo = A.range[3 * i], hi = A.range[3 * i + 1], s = A.range[3 * i + 2];
    long long *c = A.cnt + p * (A.B + 3);
    for (long long t = 0; t < A.len; ++t) {
        const double v = yp[t * A.ny];
        c[meas_hist_bin(A.mode == MEAS_HIST_ABS ? fabs(v) : v, lo, hi, s, A.B)] += 1;
    }
}

// events: every (instance, row, level) triple is a two-state automaton over the window's samples (the contract of
// include/acme_hip.h); cnt is [n * nrows * C][5] (RISE, FALL, HIGH, LOW, UNKNOWN), idx [n * nrows * C][2][E + 1], ab
// [n * nrows * C][2][E + 1][2] in the result's order, lev [2][C][n] (lo, then hi), state [n * nrows * C] and prev [n * nrows]
// (the last window sample's value) the carries
constexpr int MEAS_MAX_EVENT_LEVELS = 8, MEAS_MAX_EVENT_SLOTS = 16;
constexpr long long MEAS_MAX_EVENTS = 1ll << 24;        // N nrows C (E + 1) records per direction at most
constexpr int MEAS_EV_UNKNOWN = 0, MEAS_EV_LOW = 1, MEAS_EV_HIGH = 2;
constexpr int MEAS_EVENTS_WAVES = 4;        // pairs (one wave each) per block
constexpr int MEAS_EVENTS_AHEAD = 8;        // rounds whose loads a wave has in flight

struct MeasEventsArgs {
    const double *y;            // instance i, sample t, row r at y[(i * pitch + t0 + t) * ny + r]
    const double *lev;          // [2][C][n]
    long long *cnt, *idx;
    double *ab;
    int *state;
    double *prev;
    long long n, len, pitch, t0, m0;    // m0: the chunk's first sample is number m0 >= 0 of the window
    int C, E, ny, nrows;
    unsigned char row[64];      // the measured rows, ascending
};

// THE MASK ALGEBRA of one round of up to 64 consecutive samples, bit l = sample l: S1 the samples with v >= hi, S0 those with
// !(v >= hi) && v <= lo, `valid` the round's samples (bits from 0 up, S0 and S1 inside them), `state` the state before bit 0.
// The state after sample l is that of the highest set bit of S0 | S1 at or below l, the carried one if there is none -- the
// carry chain of an ADDITION: generate S1, propagate ~(S0 | S1), carry in state == HIGH.  In x = ~S0 + S1 + carry-in the
// carry INTO bit l is bit l of x ^ propagate: the samples that find the state HIGH; the same with S0 and S1 exchanged gives
// those that find it LOW.  No loop, no floating point.
struct MeasEventsMasks {
    unsigned long long rise, fall, high, low, unknown;      // events AT a sample; the state AFTER a sample
    int carry;                                              // the state after the last valid sample
};
ACME_HD inline MeasEventsMasks meas_events_masks(unsigned long long S0, unsigned long long S1, int state, unsigned long long valid) {
    const unsigned long long keep = ~(S0 | S1);
    // (LOW is 1 and HIGH 2: the carries in and the state out are the state's two bits)
    const unsigned long long was_high = (~S0 + S1 + (unsigned long long)(state >> 1 & 1)) ^ keep;
    const unsigned long long was_low = (~S1 + S0 + (unsigned long long)(state & 1)) ^ keep;
    const unsigned long long high = S1 | (keep & was_high), low = S0 | (keep & was_low);
    MeasEventsMasks K;
    K.rise = was_low & S1;
    K.fall = was_high & S0;
    K.high = high & valid;
    K.low = low & valid;
    K.unknown = ~(high | low) & valid;
    K.carry = (int)(high >> 63) << 1 | (int)(low >> 63);    // (keep above the valid bits hands the state up to bit 63)
    return K;
}

// the record of one event of a direction that has had `before` events: one of the first E slots of idx [E + 1], ab [E + 1][2]
// while there is room (slot E, the last event, is the caller's: a register on the device)
ACME_HD inline void meas_events_slot(long long *idx, double *ab, int E, long long before, long long m, double a, double b) {
    if (before < E) {
        idx[before] = m;
        ab[2 * before] = a;
        ab[2 * before + 1] = b;
    }
}

// one pair over the chunk, level after level, sample after sample: the contract's loop as it stands (the non-HIP backend's
// default walk)
inline void meas_events_chain(const MeasEventsArgs &A, long long p) {
    const long long i = p / A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    for (int c = 0; c < A.C; ++c) {
        const long long q = p * A.C + c;
        const double lo = A.lev[c * A.n + i], hi = A.lev[(A.C + c) * A.n + i];
        long long *cnt = A.cnt + q * 5, *idx = A.idx + q * 2 * (A.E + 1);
        double *ab = A.ab + q * 4 * (A.E + 1);
        int state = A.state[q];
        double before = A.prev[p];
        for (long long t = 0; t < A.len; ++t) {
            const double v = yp[t * A.ny];
            const int next = v >= hi ? MEAS_EV_HIGH : v <= lo ? MEAS_EV_LOW : state;
            const int d = state == MEAS_EV_LOW && next == MEAS_EV_HIGH ? 0 : state == MEAS_EV_HIGH && next == MEAS_EV_LOW ? 1 : -1;
            if (d >= 0) {
                long long *id = idx + d * (A.E + 1);
                double *abd = ab + d * 2 * (A.E + 1);
                meas_events_slot(id, abd, A.E, cnt[d], A.m0 + t, before, v);
                id[A.E] = A.m0 + t;
                abd[2 * A.E] = before;
                abd[2 * A.E + 1] = v;
                cnt[d] += 1;
            }
            cnt[next == MEAS_EV_HIGH ? 2 : next == MEAS_EV_LOW ? 3 : 4] += 1;
            state = next;
            before = v;
        }
        A.state[q] = state;
    }
    if (A.len > 0) A.prev[p] = yp[(A.len - 1) * A.ny];
}

// the same pair in ROUNDS of 64 samples through meas_events_masks and meas_events_slot, the two masks formed by a loop in
// place of the device's ballots: the algebra acme_meas_events_kernel runs, for the non-HIP backend (ACME_EVENTS_WALK=mask)
inline void meas_events_mask_walk(const MeasEventsArgs &A, long long p) {
    const long long i = p / A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    double carried = A.prev[p];
    for (long long tb = 0; tb < A.len; tb += 64) {
        const int nv = A.len - tb < 64 ? (int)(A.len - tb) : 64;
        const unsigned long long valid = nv == 64 ? ~0ull : (1ull << nv) - 1;
        for (int c = 0; c < A.C; ++c) {
            const long long q = p * A.C + c;
            const double lo = A.lev[c * A.n + i], hi = A.lev[(A.C + c) * A.n + i];
            unsigned long long S0 = 0, S1 = 0;
            for (int l = 0; l < nv; ++l) {
                const double v = yp[(tb + l) * A.ny];
                const bool ge = v >= hi;
                S1 |= (unsigned long long)ge << l;
                S0 |= (unsigned long long)(!ge && v <= lo) << l;
            }
            const MeasEventsMasks K = meas_events_masks(S0, S1, A.state[q], valid);
            long long *cnt = A.cnt + q * 5;
            for (int d = 0; d < 2; ++d) {
                const unsigned long long ev = d ? K.fall : K.rise;
                long long *id = A.idx + (q * 2 + d) * (A.E + 1);
                double *abd = A.ab + (q * 2 + d) * 2 * (A.E + 1);
                for (int l = 0; l < nv; ++l) {
                    if (!(ev >> l & 1)) continue;
                    const long long ord = cnt[d] + __builtin_popcountll(ev & ((1ull << l) - 1));    // events so far + those below
                    const double a = l ? yp[(tb + l - 1) * A.ny] : carried, b = yp[(tb + l) * A.ny];
                    meas_events_slot(id, abd, A.E, ord, A.m0 + tb + l, a, b);
                    if (!(ev >> l >> 1)) {      // the round's last event of the direction
                        id[A.E] = A.m0 + tb + l;
                        abd[2 * A.E] = a;
                        abd[2 * A.E + 1] = b;
                    }
                }
                cnt[d] += __builtin_popcountll(ev);
            }
            cnt[2] += __builtin_popcountll(K.high);
            cnt[3] += __builtin_popcountll(K.low);
            cnt[4] += __builtin_popcountll(K.unknown);
            A.state[q] = K.carry;
        }
        carried = yp[(tb + nv - 1) * A.ny];
    }
    if (A.len > 0) A.prev[p] = carried;
}

// weighting: the slice's n base-rate samples of every measured row through the cascade, the weighted samples packed
constexpr int MEAS_MAX_WEIGHT_SECTIONS = 8;
constexpr int MEAS_WEIGHT_WAVES = 4;        // the waves of a block that stage a tile jointly (acme_meas_weight_kernel)

struct MeasWeightArgs {
    const double *y;            // instance i, sample t, row r at y[(i * pitch + t) * ny + r]
    double *w;                  // [n][len][nrows]: instance i, sample t, j-th measured row at w[(i * len + t) * nrows + j]
    double *state;              // [2 S][n * nrows]: plane 2 k the s1 of section k, plane 2 k + 1 its s2
    long long n, len, pitch;
    int ny, nrows, S;
    double sos[MEAS_MAX_WEIGHT_SECTIONS][5];    // b0 b1 b2 a1 a2
    unsigned char row[64];      // the measured rows, ascending
};

// one section on one sample: the contract's four lines (every product and every sum rounded on its own)
ACME_HD ACME_NO_CONTRACT_FN inline double meas_weight_section(const double *c, double x, double &s1, double &s2) {
    ACME_NO_CONTRACT
    const double b0x = c[0] * x;
    const double v = b0x + s1;
    const double b1x = c[1] * x, a1v = c[3] * v;
    const double d1 = b1x - a1v;
    s1 = d1 + s2;
    const double b2x = c[2] * x, a2v = c[4] * v;
    s2 = b2x - a2v;
    return v;
}

// one pair over the slice, sample after sample: the contract of include/acme_hip.h as a plain loop (the reference order every
// backend keeps)
ACME_HD inline void meas_weight_chain(const MeasWeightArgs &A, long long p) {
    const long long Pn = A.n * A.nrows, i = p / A.nrows, j = p - i * A.nrows;
    const double *yp = A.y + i * A.pitch * A.ny + A.row[j];
    double *wp = A.w + i * A.len * A.nrows + j;
    double s1[MEAS_MAX_WEIGHT_SECTIONS], s2[MEAS_MAX_WEIGHT_SECTIONS];
    for (int k = 0; k < A.S; ++k) { s1[k] = A.state[2 * k * Pn + p]; s2[k] = A.state[(2 * k + 1) * Pn + p]; }
    for (long long t = 0; t < A.len; ++t) {
        double x = yp[t * A.ny];
        for (int k = 0; k < A.S; ++k) x = meas_weight_section(A.sos[k], x, s1[k], s2[k]);
        wp[t * A.nrows] = x;
    }
    for (int k = 0; k < A.S; ++k) { A.state[2 * k * Pn + p] = s1[k]; A.state[(2 * k + 1) * Pn + p] = s2[k]; }
}

// one unit of one pair over the chunk, sample after sample (the reference order every backend keeps)
ACME_HD inline void meas_chain(const MeasArgs &A, long long p, int u) {
    const long long P = A.n * A.nrows;
    const long long i = p / A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    double *acc = A.acc + p;
    if (u == 0) {
        double s = acc[0], q = acc[P], mn = acc[2 * P], mx = acc[3 * P];
        for (long long t = 0; t < A.len; ++t) {
            const double v = yp[t * A.ny];
            s += v;
            q = fma(v, v, q);
            mn = meas_min(mn, v);
            mx = meas_max(mx, v);
        }
        acc[0] = s; acc[P] = q; acc[2 * P] = mn; acc[3 * P] = mx;
        return;
    }
    const double *tw = A.tw + 2 * (u - 1) * A.len;
    double c = acc[(2 + 2 * u) * P], sn = acc[(3 + 2 * u) * P];
    for (long long t = 0; t < A.len; ++t) {
        const double v = yp[t * A.ny];
        c = fma(v, tw[2 * t], c);
        sn = fma(v, tw[2 * t + 1], sn);
    }
    acc[(2 + 2 * u) * P] = c;
    acc[(3 + 2 * u) * P] = sn;
}

// series: one unit of one pair over the chunk (tw: the table row [H][len] of the pair's group), sample after sample into
// the sample's window; a window's first sample starts from meas_init
ACME_HD inline void meas_series_chain(const MeasArgs &A, const MeasSeries &S, const double *twg, long long p, int u) {
    const long long P = A.n * A.nrows;
    const long long i = p / A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    const double *tw = twg + 2 * (u > 0 ? u - 1 : 0) * A.len;
    for (long long t = 0; t < A.len; ++t) {
        long long w, m;
        if (!meas_series_at(S, S.s0 + t, &w, &m)) continue;
        double *acc = A.acc + w * (4 + 2 * A.H) * P + p;
        const double v = yp[t * A.ny];
        if (u == 0) {
            if (m == 0) { acc[0] = 0.0; acc[P] = 0.0; acc[2 * P] = INFINITY; acc[3 * P] = -INFINITY; }
            acc[0] += v;
            acc[P] = fma(v, v, acc[P]);
            acc[2 * P] = meas_min(acc[2 * P], v);
            acc[3 * P] = meas_max(acc[3 * P], v);
        } else {
            double *c = acc + (2 + 2 * u) * P, *sn = acc + (3 + 2 * u) * P;
            if (m == 0) { *c = 0.0; *sn = 0.0; }
            *c = fma(v, tw[2 * t], *c);
            *sn = fma(v, tw[2 * t + 1], *sn);
        }
    }
}

// waves per block and blocks along y for H harmonics: H + 1 units, at most MEAS_MAX_WAVES waves a block
inline void meas_shape(int H, int *waves, int *groups) {
    const int U = H + 1;
    *groups = (U + MEAS_MAX_WAVES - 1) / MEAS_MAX_WAVES;
    *waves = (U + *groups - 1) / *groups;
}

// samples per step of a per-instance measurement: F groups, H harmonics, `budget` bytes of table
inline long long meas_pi_chunk(long long F, int H, long long budget) {
    if (H == 0) return MEAS_CHUNK;
    long long len = budget / (F * H * 16) / MEAS_TILE * MEAS_TILE;
    if (len > MEAS_CHUNK) len = MEAS_CHUNK;
    return len < MEAS_TILE ? MEAS_TILE : len;
}

// the plan of a per-instance measurement from the instances' groups grp[n] (0 ... F - 1): perm, sgrp, wgrp as MeasPiArgs
// describes them.  Whole waves of one group first, the remainders packed behind them, both in group order and, inside a
// group, in pair order.
template <class VL, class VI>
inline void meas_pi_plan(const VI &grp, long long n, int nrows, int F, VL *perm, VI *sgrp, VI *wgrp) {
    const long long P = n * nrows;
    std::vector<long long> cnt((size_t)F, 0), at((size_t)F + 1, 0);
    for (long long i = 0; i < n; ++i) cnt[(size_t)grp[(size_t)i]] += nrows;
    // slots of the whole waves, then of the remainders
    std::vector<long long> full((size_t)F), rest((size_t)F);
    long long s = 0;
    for (int g = 0; g < F; ++g) { full[(size_t)g] = s; s += cnt[(size_t)g] / 64 * 64; }
    for (int g = 0; g < F; ++g) { rest[(size_t)g] = s; s += cnt[(size_t)g] % 64; }
    perm->assign((size_t)P, 0);
    sgrp->assign((size_t)P, 0);
    std::vector<long long> seen((size_t)F, 0);
    for (long long p = 0; p < P; ++p) {
        const int g = grp[(size_t)(p / nrows)];
        const long long k = seen[(size_t)g]++, whole = cnt[(size_t)g] / 64 * 64;
        const long long slot = k < whole ? full[(size_t)g] + k : rest[(size_t)g] + (k - whole);
        (*perm)[(size_t)slot] = p;
        (*sgrp)[(size_t)slot] = g;
    }
    wgrp->assign((size_t)((P + 63) / 64), 0);
    for (long long w = 0; w * 64 < P; ++w) {
        int g = (*sgrp)[(size_t)(w * 64)];
        for (long long q = w * 64; q < P && q < w * 64 + 64; ++q)
            if ((*sgrp)[(size_t)q] != g) g = -1;
        (*wgrp)[(size_t)w] = g;
    }
}

}  // namespace acme

// ---- launchers ---------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void acme_meas_tw_kernel(acme::MeasTwArgs A) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < A.H * A.len) acme::meas_tw(A, idx);
}

__device__ inline double acme_meas_bcast(double v, int l) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// block: 64 pairs x blockDim.x / 64 units (unit = blockIdx.y * waves + wave); every wave helps stage the tiles
__global__ __launch_bounds__(1024) void acme_meas_kernel(acme::MeasArgs A) {
    using namespace acme;
    __shared__ double tile[64][MEAS_TILE + 1];          // [pair][sample]: column reads by lane hit distinct banks
    __shared__ long long base[64];                      // a pair's first element of the chunk in y
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long long P = A.n * A.nrows, p0 = (long long)blockIdx.x * 64, p = p0 + lane;
    const int u = blockIdx.y * nw + w;
    const bool mine = u <= A.H && p < P;
    if (threadIdx.x < 64) {
        const long long q = p0 + threadIdx.x;
        if (q < P) {
            const long long i = q / A.nrows;
            base[threadIdx.x] = (i * A.pitch + A.t0) * A.ny + A.row[q - i * A.nrows];
        }
    }
    // the unit's accumulators (unit 0: sum, sq, min, max; unit h: C_h, S_h)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const int ia = u == 0 ? 0 : 2 + 2 * u;
    if (mine) {
        a0 = A.acc[ia * P + p];
        a1 = A.acc[(ia + 1) * P + p];
        if (u == 0) { a2 = A.acc[2 * P + p]; a3 = A.acc[3 * P + p]; }
    }
    const double *tw = A.tw + 2 * (long long)(u > 0 ? u - 1 : 0) * A.len;
    for (long long tb = 0; tb < A.len; tb += MEAS_TILE) {
        const int nt = (int)(A.len - tb < MEAS_TILE ? A.len - tb : MEAS_TILE);
        __syncthreads();                                // (the previous tile has been read by every wave)
        for (int pp = w; pp < 64; pp += nw)            // wave pp: pair pp's samples, one per lane -- contiguous for ny = 1
            if (p0 + pp < P && lane < nt) tile[pp][lane] = A.y[base[pp] + (tb + lane) * A.ny];
        __syncthreads();
        if (u > A.H) continue;
        if (u == 0) {
            for (int t = 0; t < nt; ++t) {
                const double v = tile[lane][t];
                a0 += v;
                a1 = fma(v, v, a1);
                a2 = meas_min(a2, v);
                a3 = meas_max(a3, v);
            }
        } else {
            double cl = 0.0, sl = 0.0;                 // lane t holds sample tb + t's twiddle
            if (lane < nt) { cl = tw[2 * (tb + lane)]; sl = tw[2 * (tb + lane) + 1]; }
            if (nt == MEAS_TILE) {                     // (a whole tile: a fixed trip count the compiler unrolls)
#pragma unroll 8
                for (int t = 0; t < MEAS_TILE; ++t) {
                    const double v = tile[lane][t];
                    a0 = fma(v, acme_meas_bcast(cl, t), a0);
                    a1 = fma(v, acme_meas_bcast(sl, t), a1);
                }
            } else {
                for (int t = 0; t < nt; ++t) {
                    const double v = tile[lane][t];
                    a0 = fma(v, acme_meas_bcast(cl, t), a0);
                    a1 = fma(v, acme_meas_bcast(sl, t), a1);
                }
            }
        }
    }
    if (mine) {
        A.acc[ia * P + p] = a0;
        A.acc[(ia + 1) * P + p] = a1;
        if (u == 0) { A.acc[2 * P + p] = a2; A.acc[3 * P + p] = a3; }
    }
}
__global__ __launch_bounds__(256) void acme_meas_pi_tw_kernel(acme::MeasPiTwArgs A) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < (long long)A.F * A.H * A.len) acme::meas_pi_tw(A, idx);
}

// per-instance fundamentals: acme_meas_kernel with the pairs taken through the plan's permutation; a uniform wave reads its
// group's table row and broadcasts, a mixed wave's lanes read their own rows (16-byte loads, eight samples ahead)
__global__ __launch_bounds__(1024) void acme_meas_pi_kernel(acme::MeasPiArgs B) {
    using namespace acme;
    const MeasArgs &A = B.A;
    __shared__ double tile[64][MEAS_TILE + 1];          // [slot][sample]: column reads by lane hit distinct banks
    __shared__ long long base[64];                      // a slot's pair: its first element of the chunk in y
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long long P = A.n * A.nrows, p0 = (long long)blockIdx.x * 64;
    const int u = blockIdx.y * nw + w;
    const bool mine = u <= A.H && p0 + lane < P;
    const long long p = p0 + lane < P ? B.perm[p0 + lane] : 0;
    if (threadIdx.x < 64 && p0 + lane < P) {
        const long long i = p / A.nrows;
        base[lane] = (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const int ia = u == 0 ? 0 : 2 + 2 * u;
    if (mine) {
        a0 = A.acc[ia * P + p];
        a1 = A.acc[(ia + 1) * P + p];
        if (u == 0) { a2 = A.acc[2 * P + p]; a3 = A.acc[3 * P + p]; }
    }
    const int wg = B.wgrp[blockIdx.x];                 // (wave-uniform: one value per block)
    const int g = wg >= 0 ? wg : mine ? B.sgrp[p0 + lane] : 0;
    const double *tw = A.tw + 2 * ((long long)g * A.H + (u > 0 ? u - 1 : 0)) * A.len;
    for (long long tb = 0; tb < A.len; tb += MEAS_TILE) {
        const int nt = (int)(A.len - tb < MEAS_TILE ? A.len - tb : MEAS_TILE);
        __syncthreads();                                // (the previous tile has been read by every wave)
        for (int pp = w; pp < 64; pp += nw)
            if (p0 + pp < P && lane < nt) tile[pp][lane] = A.y[base[pp] + (tb + lane) * A.ny];
        __syncthreads();
        if (u > A.H) continue;
        if (u == 0) {
            for (int t = 0; t < nt; ++t) {
                const double v = tile[lane][t];
                a0 += v;
                a1 = fma(v, v, a1);
                a2 = meas_min(a2, v);
                a3 = meas_max(a3, v);
            }
        } else if (wg >= 0) {
            double cl = 0.0, sl = 0.0;                 // lane t holds sample tb + t's twiddle
            if (lane < nt) { cl = tw[2 * (tb + lane)]; sl = tw[2 * (tb + lane) + 1]; }
            if (nt == MEAS_TILE) {
#pragma unroll 8
                for (int t = 0; t < MEAS_TILE; ++t) {
                    const double v = tile[lane][t];
                    a0 = fma(v, acme_meas_bcast(cl, t), a0);
                    a1 = fma(v, acme_meas_bcast(sl, t), a1);
                }
            } else {
                for (int t = 0; t < nt; ++t) {
                    const double v = tile[lane][t];
                    a0 = fma(v, acme_meas_bcast(cl, t), a0);
                    a1 = fma(v, acme_meas_bcast(sl, t), a1);
                }
            }
        } else if (mine) {
            const double2 *tl = reinterpret_cast<const double2 *>(tw) + tb;    // (16-byte aligned: pairs of a hipMalloc'ed table)
            if (nt == MEAS_TILE) {
                double2 nx[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) nx[k] = tl[k];
#pragma unroll
                for (int t = 0; t < MEAS_TILE; t += 8) {
                    double2 cs[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) cs[k] = nx[k];
                    if (t + 8 < MEAS_TILE) {           // the next eight samples' loads are in flight under this chain
#pragma unroll
                        for (int k = 0; k < 8; ++k) nx[k] = tl[t + 8 + k];
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const double v = tile[lane][t + k];
                        a0 = fma(v, cs[k].x, a0);
                        a1 = fma(v, cs[k].y, a1);
                    }
                }
            } else {
                for (int t = 0; t < nt; ++t) {
                    const double2 cs = tl[t];
                    const double v = tile[lane][t];
                    a0 = fma(v, cs.x, a0);
                    a1 = fma(v, cs.y, a1);
                }
            }
        }
    }
    if (mine) {
        A.acc[ia * P + p] = a0;
        A.acc[(ia + 1) * P + p] = a1;
        if (u == 0) { A.acc[2 * P + p] = a2; A.acc[3 * P + p] = a3; }
    }
}
__global__ __launch_bounds__(256) void acme_meas_bins_tw_kernel(acme::MeasBinsTwArgs A) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < (long long)A.F * A.B * A.len) acme::meas_bins_tw(A, idx);
}
__global__ __launch_bounds__(256) void acme_meas_series_tw_kernel(acme::MeasSeriesTwArgs A) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < (long long)A.F * A.H * A.len) acme::meas_series_tw(A, idx);
}

// series: acme_meas_kernel (PI = false) / acme_meas_pi_kernel (PI = true) over a chunk that several windows share.  (wt, mt):
// window and window-relative number of the tile's first sample, kept by every wave alike; (w, m) walk the tile's sub-ranges.
// `open`: the registers hold window w's accumulators (they are stored when the window, or the chunk, ends).
template <bool PI>
__global__ __launch_bounds__(1024) void acme_meas_series_kernel(acme::MeasSeriesArgs G) {
    using namespace acme;
    const MeasArgs &A = G.B.A;
    const MeasSeries &S = G.S;
    __shared__ double tile[64][MEAS_TILE + 1];          // [slot][sample]: column reads by lane hit distinct banks
    __shared__ long long base[64];                      // a slot's pair: its first element of the chunk in y
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long long P = A.n * A.nrows, p0 = (long long)blockIdx.x * 64;
    const int u = blockIdx.y * nw + wv;
    const bool mine = u <= A.H && p0 + lane < P;
    const long long p = p0 + lane < P ? (PI ? G.B.perm[p0 + lane] : p0 + lane) : 0;
    if (threadIdx.x < 64 && p0 + lane < P) {
        const long long i = p / A.nrows;
        base[lane] = (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    }
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const int ia = u == 0 ? 0 : 2 + 2 * u;
    const long long slot = (long long)(4 + 2 * A.H) * P;
    const int wg = PI ? G.B.wgrp[blockIdx.x] : 0;      // (wave-uniform: one value per block)
    const int g = !PI ? 0 : wg >= 0 ? wg : mine ? G.B.sgrp[p0 + lane] : 0;
    const double *tw = A.tw + 2 * ((long long)g * A.H + (u > 0 ? u - 1 : 0)) * A.len;
    long long wt = S.s0 / S.hop, mt = S.s0 - wt * S.hop;
    bool open = false;
    long long wo = 0;                                   // the open window
    for (long long tb = 0; tb < A.len; tb += MEAS_TILE) {
        const int nt = (int)(A.len - tb < MEAS_TILE ? A.len - tb : MEAS_TILE);
        long long w = wt, m = mt;
        mt += nt;                                       // (the next tile's first sample)
        if (mt >= S.hop) { const long long d = mt / S.hop; wt += d; mt -= d * S.hop; }
        // the tile holds a sample of a window: its first sample does, or a later window begins inside it
        if (!(w < S.W && (m < S.win || (m + nt > S.hop && w + 1 < S.W)))) continue;
        __syncthreads();                                // (the previous tile has been read by every wave)
        for (int pp = wv; pp < 64; pp += nw)
            if (p0 + pp < P && lane < nt) tile[pp][lane] = A.y[base[pp] + (tb + lane) * A.ny];
        __syncthreads();
        if (u > A.H) continue;
        for (int pos = 0; pos < nt && w < S.W;) {
            if (m >= S.win) {                           // a gap: to the next window's first sample, or the tile's end
                const long long adv = S.hop - m < nt - pos ? S.hop - m : nt - pos;
                pos += (int)adv;
                m += adv;
                if (m == S.hop) { m = 0; ++w; }
                continue;
            }
            const int seg = (int)(S.win - m < nt - pos ? S.win - m : nt - pos), end = pos + seg;
            if (!open) {
                open = true;
                wo = w;
                if (m == 0) {                           // the window's first sample: meas_init
                    a0 = 0.0; a1 = 0.0; a2 = INFINITY; a3 = -INFINITY;
                } else if (mine) {                      // it continues from an earlier chunk
                    const double *acc = A.acc + w * slot + p;
                    a0 = acc[ia * P];
                    a1 = acc[(ia + 1) * P];
                    if (u == 0) { a2 = acc[2 * P]; a3 = acc[3 * P]; }
                }
            }
            if (u == 0) {
                for (int t = pos; t < end; ++t) {
                    const double v = tile[lane][t];
                    a0 += v;
                    a1 = fma(v, v, a1);
                    a2 = meas_min(a2, v);
                    a3 = meas_max(a3, v);
                }
            } else if (!PI || wg >= 0) {
                double cl = 0.0, sl = 0.0;             // lane t holds sample tb + t's twiddle (the sub-range's only)
                if (lane >= pos && lane < end) { cl = tw[2 * (tb + lane)]; sl = tw[2 * (tb + lane) + 1]; }
                if (seg == MEAS_TILE) {                // (a whole tile: a fixed trip count the compiler unrolls)
#pragma unroll 8
                    for (int t = 0; t < MEAS_TILE; ++t) {
                        const double v = tile[lane][t];
                        a0 = fma(v, acme_meas_bcast(cl, t), a0);
                        a1 = fma(v, acme_meas_bcast(sl, t), a1);
                    }
                } else {
                    for (int t = pos; t < end; ++t) {
                        const double v = tile[lane][t];
                        a0 = fma(v, acme_meas_bcast(cl, t), a0);
                        a1 = fma(v, acme_meas_bcast(sl, t), a1);
                    }
                }
            } else if (mine) {
                const double2 *tl = reinterpret_cast<const double2 *>(tw) + tb;    // (16-byte aligned: pairs of a hipMalloc'ed table)
                if (seg == MEAS_TILE) {
                    double2 nx[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) nx[k] = tl[k];
#pragma unroll
                    for (int t = 0; t < MEAS_TILE; t += 8) {
                        double2 cs[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) cs[k] = nx[k];
                        if (t + 8 < MEAS_TILE) {       // the next eight samples' loads are in flight under this chain
#pragma unroll
                            for (int k = 0; k < 8; ++k) nx[k] = tl[t + 8 + k];
                        }
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const double v = tile[lane][t + k];
                            a0 = fma(v, cs[k].x, a0);
                            a1 = fma(v, cs[k].y, a1);
                        }
                    }
                } else {
                    for (int t = pos; t < end; ++t) {
                        const double2 cs = tl[t];
                        const double v = tile[lane][t];
                        a0 = fma(v, cs.x, a0);
                        a1 = fma(v, cs.y, a1);
                    }
                }
            }
            pos = end;
            m += seg;
            if (m == S.win) {                           // the window's last sample: its slot, coalesced along the pairs
                if (mine) {
                    double *acc = A.acc + w * slot + p;
                    acc[ia * P] = a0;
                    acc[(ia + 1) * P] = a1;
                    if (u == 0) { acc[2 * P] = a2; acc[3 * P] = a3; }
                }
                open = false;
                if (m == S.hop) { m = 0; ++w; }
            }
        }
    }
    if (open && mine) {                                 // the chunk ends inside the window
        double *acc = A.acc + wo * slot + p;
        acc[ia * P] = a0;
        acc[(ia + 1) * P] = a1;
        if (u == 0) { acc[2 * P] = a2; acc[3 * P] = a3; }
    }
}

// fold: U blocks of 64 of the chunk's first `cover` samples from cb on, K periods a step.  Lane l of block u owns sample
// c = cb + 64 u + l and its slot; the loads of a step are issued together, the additions follow per slot in sample order.
template <int U, int K>
__device__ inline void acme_meas_fold_span(const double *yp, double *f, long long cb, long long cover, long long len,
                                           long long ph, long long P, int ny, int lane) {
    double a[U];
    long long s[U];
    bool on[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const long long c = cb + 64 * u + lane;
        on[u] = c < cover;
        s[u] = ph + c < P ? ph + c : ph + c - P;        // (ph < P and c < P: one wrap at most)
        a[u] = on[u] ? f[s[u]] : 0.0;
    }
    for (long long tb = cb; tb < len; tb += K * P) {
        double v[K][U];
        bool h[K][U];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long t = tb + k * P + 64 * u + lane;
                h[k][u] = on[u] && t < len;
                v[k][u] = h[k][u] ? yp[t * ny] : 0.0;
            }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (h[k][u]) a[u] += v[k][u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
        if (on[u]) f[s[u]] = a[u];
}

// block: MEAS_FOLD_WAVES pairs, a wave each (the period, the phase and the pair's addresses are wave-uniform)
__global__ __launch_bounds__(64 * acme::MEAS_FOLD_WAVES) void acme_meas_fold_kernel(acme::MeasFoldArgs A) {
    using namespace acme;
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * MEAS_FOLD_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (p >= A.n * A.nrows) return;
    const long long i = p / A.nrows, P = A.per[i];
    const long long ph = A.m0 % P;                      // once per wave, in 64-bit integers
    const long long cover = A.len < P ? A.len : P;      // the slots the chunk reaches: its first min(len, P) samples'
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    double *f = A.fold + p * A.pmax;
    long long cb = 0;
    for (; cover - cb > 64; cb += 256) acme_meas_fold_span<4, 2>(yp, f, cb, cover, A.len, ph, P, A.ny, lane);
    if (cb < cover) acme_meas_fold_span<1, 8>(yp, f, cb, cover, A.len, ph, P, A.ny, lane);
}

// spectrum: a block of 256 lanes per pair.  The transform's vector lives in LDS as two arrays of doubles (re, im), element i
// at i + i / 32: one double of padding per 32 (a bank row of the 8-byte reads), so that the four elements of a lane at the
// power-of-two strides of the early passes, and the bit-reversed stores of the load, spread over the banks.  A pass keeps
// two stages in registers: lane work item j owns the elements i0, i0 + h, i0 + 2h, i0 + 3h (i0 = (j / h) 4h + j mod h) and
// runs the four radix-2 butterflies of stages q + 1 (half-size h) and q + 2 (half-size 2h) on them; an odd log2 L ends in one
// pass of plain butterflies at h = L / 2.  The first pass never reads the imaginary array (it holds nothing yet: the zeros
// are formed in registers).  L < 1024 fills the block with G = 1024 / L segments side by side; the bins' owners then add the
// G power spectra in segment order.  A lane owns bins k = lane + 256 b and keeps their sums in registers over the chunk.
// The carry is read by the loads only, every load is followed by a barrier of the block, and the rewrite comes behind the
// last of them.
__device__ inline void acme_meas_spec_bf(double &ar, double &ai, double &br, double &bi, double wr, double wi) {
    ACME_NO_CONTRACT
    const double p0 = wr * br, p1 = wi * bi, p2 = wr * bi, p3 = wi * br;
    const double tr = p0 - p1, ti = p2 + p3;
    br = ar - tr;
    bi = ai - ti;
    ar = ar + tr;
    ai = ai + ti;
}
template <int LOG2L>
__global__ __launch_bounds__(256) void acme_meas_spectrum_kernel(acme::MeasSpecArgs A) {
    ACME_NO_CONTRACT
    using namespace acme;
    constexpr int L = 1 << LOG2L, Q = L / 4, G = Q >= 256 ? 1 : 256 / Q, PITCH = L + L / 32, NB = (L / 2 + 256) / 256;
    __shared__ double sre[G * PITCH], sim[G * PITCH];
    const int tid = threadIdx.x;
    const long long p = blockIdx.x, i = p / A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    double *carry = A.carry + p * L, *acc = A.acc + p * (L / 2 + 1);
    long long s_lo, s_hi;
    meas_spec_segments(A.m0, A.len, L, A.hop, &s_lo, &s_hi);
    double a[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) a[b] = s_lo <= s_hi && tid + 256 * b <= L / 2 ? acc[tid + 256 * b] : 0.0;
    for (long long s0 = s_lo; s0 <= s_hi; s0 += G) {
        // x = w y of the round's segments, stored in bit-reversed order
        for (int e = tid; e < G * L; e += 256) {
            const int g = e >> LOG2L, j = e & (L - 1);
            if (s0 + g > s_hi) continue;
            const long long m = (s0 + g) * A.hop + j;
            const double v = m >= A.m0 ? yp[(m - A.m0) * A.ny] : carry[m & (L - 1)];
            const int r = (int)(__brev((unsigned)j) >> (32 - LOG2L));
            sre[g * PITCH + r + (r >> 5)] = A.w[j] * v;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q + 2 <= LOG2L; q += 2) {
            const int h = 1 << q;
            for (int e = tid; e < G * Q; e += 256) {
                const int g = e >> (LOG2L - 2), j = e & (Q - 1), r = j & (h - 1), i0 = ((j >> q) << (q + 2)) + r;
                if (s0 + g > s_hi) continue;
                double *re = sre + g * PITCH, *im = sim + g * PITCH;
                int at[4];
                double xr[4], xi[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    at[c] = i0 + c * h + ((i0 + c * h) >> 5);
                    xr[c] = re[at[c]];
                    xi[c] = q == 0 ? 0.0 : im[at[c]];
                }
                const double *ta = A.tw + 2 * ((long long)r << (LOG2L - 1 - q));
                const double *tb = A.tw + 2 * ((long long)r << (LOG2L - 2 - q));
                const double *tc = A.tw + 2 * ((long long)(r + h) << (LOG2L - 2 - q));
                const double ar = ta[0], ai = ta[1], br = tb[0], bi = tb[1], cr = tc[0], ci = tc[1];
                acme_meas_spec_bf(xr[0], xi[0], xr[1], xi[1], ar, ai);
                acme_meas_spec_bf(xr[2], xi[2], xr[3], xi[3], ar, ai);
                acme_meas_spec_bf(xr[0], xi[0], xr[2], xi[2], br, bi);
                acme_meas_spec_bf(xr[1], xi[1], xr[3], xi[3], cr, ci);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    re[at[c]] = xr[c];
                    im[at[c]] = xi[c];
                }
            }
            __syncthreads();
        }
        if (LOG2L & 1) {                                // the last stage on its own: h = L / 2, twiddle index i
            for (int e = tid; e < G * (L / 2); e += 256) {
                const int g = e >> (LOG2L - 1), j = e & (L / 2 - 1);
                if (s0 + g > s_hi) continue;
                double *re = sre + g * PITCH, *im = sim + g * PITCH;
                const int a0 = j + (j >> 5), a1 = j + L / 2 + ((j + L / 2) >> 5);
                double xr0 = re[a0], xi0 = im[a0], xr1 = re[a1], xi1 = im[a1];
                acme_meas_spec_bf(xr0, xi0, xr1, xi1, A.tw[2 * j], A.tw[2 * j + 1]);
                re[a0] = xr0;
                im[a0] = xi0;
                re[a1] = xr1;
                im[a1] = xi1;
            }
            __syncthreads();
        }
        // |X_k|^2 of the round's segments into the bins' chains, in segment order
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int k = tid + 256 * b;
            if (k > L / 2) continue;
            for (int g = 0; g < G && s0 + g <= s_hi; ++g) {
                const double xr = sre[g * PITCH + k + (k >> 5)], xi = sim[g * PITCH + k + (k >> 5)];
                const double pr = xr * xr, pi = xi * xi;
                const double pw = pr + pi;
                a[b] = a[b] + pw;
            }
        }
        __syncthreads();                                // (the next round's load overwrites the vectors)
    }
    if (s_lo <= s_hi) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (tid + 256 * b <= L / 2) acc[tid + 256 * b] = a[b];
    }
    // the chunk's last min(len, L) samples into the ring (every read of it lies before a barrier above)
    for (long long t = (A.len > L ? A.len - L : 0) + tid; t < A.len; t += 256) carry[(A.m0 + t) & (L - 1)] = yp[t * A.ny];
}

// cross-spectrum: the spectrum kernel's shape -- a block of 256 lanes per pair, the padded re / im arrays, two stages a pass,
// G = 1024 / L segments side by side -- on z = w x + i w y: the load fills BOTH arrays (the real part from the input row, the
// imaginary part from the measured row, both in bit-reversed order), so the first pass reads the imaginary array like every
// other.  Behind the passes the owner of bin k = lane + 256 b reads Z at k and at n = (L - k) mod L, splits X and Y off and
// adds into four sums per bin, held in registers over the chunk.  The reads at k ascend with the lane and are free of bank
// conflicts as the spectrum's; the reads at n descend: the 32 lanes of a half wave (k = 32 a ... 32 a + 31) cover the padded
// positions of n = L - 32 a - 31 ... L - 32 a, 33 consecutive doubles less the one pad between the last two, so lanes 0 and 31
// of every half meet in one bank -- a two-way conflict on each of the two descending reads, none elsewhere.  Both rings are
// read by the loads only, every load is followed by a barrier of the block, and the rewrite comes behind the last of them.
template <int LOG2L>
__global__ __launch_bounds__(256) void acme_meas_cross_kernel(acme::MeasCrossArgs C) {
    ACME_NO_CONTRACT
    using namespace acme;
    constexpr int L = 1 << LOG2L, Q = L / 4, G = Q >= 256 ? 1 : 256 / Q, PITCH = L + L / 32, NB = (L / 2 + 256) / 256, NK = L / 2 + 1;
    __shared__ double sre[G * PITCH], sim[G * PITCH];
    const MeasSpecArgs &A = C.S;
    const int tid = threadIdx.x;
    const long long p = blockIdx.x, i = p / A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    const double *up = C.u + (i * C.upitch + A.t0) * C.nu + C.in_row;
    double *cx = A.carry + p * (2 * L), *cy = cx + L, *acc = A.acc + p * (4 * NK);
    long long s_lo, s_hi;
    meas_spec_segments(A.m0, A.len, L, A.hop, &s_lo, &s_hi);
    double axx[NB], ayy[NB], are[NB], aim[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const bool own = s_lo <= s_hi && tid + 256 * b <= L / 2;
        axx[b] = own ? acc[tid + 256 * b] : 0.0;
        ayy[b] = own ? acc[NK + tid + 256 * b] : 0.0;
        are[b] = own ? acc[2 * NK + tid + 256 * b] : 0.0;
        aim[b] = own ? acc[3 * NK + tid + 256 * b] : 0.0;
    }
    for (long long s0 = s_lo; s0 <= s_hi; s0 += G) {
        // z = w x + i w y of the round's segments, stored in bit-reversed order
        for (int e = tid; e < G * L; e += 256) {
            const int g = e >> LOG2L, j = e & (L - 1);
            if (s0 + g > s_hi) continue;
            const long long m = (s0 + g) * A.hop + j;
            const double vx = m >= A.m0 ? up[(m - A.m0) * C.nu] : cx[m & (L - 1)];
            const double vy = m >= A.m0 ? yp[(m - A.m0) * A.ny] : cy[m & (L - 1)];
            const int r = (int)(__brev((unsigned)j) >> (32 - LOG2L));
            const double wj = A.w[j];
            sre[g * PITCH + r + (r >> 5)] = wj * vx;
            sim[g * PITCH + r + (r >> 5)] = wj * vy;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q + 2 <= LOG2L; q += 2) {
            const int h = 1 << q;
            for (int e = tid; e < G * Q; e += 256) {
                const int g = e >> (LOG2L - 2), j = e & (Q - 1), r = j & (h - 1), i0 = ((j >> q) << (q + 2)) + r;
                if (s0 + g > s_hi) continue;
                double *re = sre + g * PITCH, *im = sim + g * PITCH;
                int at[4];
                double xr[4], xi[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    at[c] = i0 + c * h + ((i0 + c * h) >> 5);
                    xr[c] = re[at[c]];
                    xi[c] = im[at[c]];
                }
                const double *ta = A.tw + 2 * ((long long)r << (LOG2L - 1 - q));
                const double *tb = A.tw + 2 * ((long long)r << (LOG2L - 2 - q));
                const double *tc = A.tw + 2 * ((long long)(r + h) << (LOG2L - 2 - q));
                const double ar = ta[0], ai = ta[1], br = tb[0], bi = tb[1], cr = tc[0], ci = tc[1];
                acme_meas_spec_bf(xr[0], xi[0], xr[1], xi[1], ar, ai);
                acme_meas_spec_bf(xr[2], xi[2], xr[3], xi[3], ar, ai);
                acme_meas_spec_bf(xr[0], xi[0], xr[2], xi[2], br, bi);
                acme_meas_spec_bf(xr[1], xi[1], xr[3], xi[3], cr, ci);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    re[at[c]] = xr[c];
                    im[at[c]] = xi[c];
                }
            }
            __syncthreads();
        }
        if (LOG2L & 1) {                                // the last stage on its own: h = L / 2, twiddle index i
            for (int e = tid; e < G * (L / 2); e += 256) {
                const int g = e >> (LOG2L - 1), j = e & (L / 2 - 1);
                if (s0 + g > s_hi) continue;
                double *re = sre + g * PITCH, *im = sim + g * PITCH;
                const int a0 = j + (j >> 5), a1 = j + L / 2 + ((j + L / 2) >> 5);
                double xr0 = re[a0], xi0 = im[a0], xr1 = re[a1], xi1 = im[a1];
                acme_meas_spec_bf(xr0, xi0, xr1, xi1, A.tw[2 * j], A.tw[2 * j + 1]);
                re[a0] = xr0;
                im[a0] = xi0;
                re[a1] = xr1;
                im[a1] = xi1;
            }
            __syncthreads();
        }
        // X and Y of the round's segments split off Z, and the four products into the bins' chains, in segment order
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int k = tid + 256 * b, n = (L - k) & (L - 1);
            if (k > L / 2) continue;
            const int ak = k + (k >> 5), an = n + (n >> 5);
            for (int g = 0; g < G && s0 + g <= s_hi; ++g) {
                const double zrk = sre[g * PITCH + ak], zik = sim[g * PITCH + ak];
                const double zrn = sre[g * PITCH + an], zin = sim[g * PITCH + an];
                const double xr = 0.5 * (zrk + zrn), xi = 0.5 * (zik - zin);
                const double yr = 0.5 * (zik + zin), yi = 0.5 * (zrn - zrk);
                const double p0 = xr * xr, p1 = xi * xi, p2 = yr * yr, p3 = yi * yi;
                const double p4 = xr * yr, p5 = xi * yi, p6 = xr * yi, p7 = xi * yr;
                const double sxx = p0 + p1, syy = p2 + p3, sre_ = p4 + p5, sim_ = p6 - p7;
                axx[b] = axx[b] + sxx;
                ayy[b] = ayy[b] + syy;
                are[b] = are[b] + sre_;
                aim[b] = aim[b] + sim_;
            }
        }
        __syncthreads();                                // (the next round's load overwrites the vectors)
    }
    if (s_lo <= s_hi) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (tid + 256 * b <= L / 2) {
                acc[tid + 256 * b] = axx[b];
                acc[NK + tid + 256 * b] = ayy[b];
                acc[2 * NK + tid + 256 * b] = are[b];
                acc[3 * NK + tid + 256 * b] = aim[b];
            }
    }
    // the chunk's last min(len, L) samples into the rings (every read of them lies before a barrier above)
    for (long long t = (A.len > L ? A.len - L : 0) + tid; t < A.len; t += 256) {
        cx[(A.m0 + t) & (L - 1)] = up[t * C.nu];
        cy[(A.m0 + t) & (L - 1)] = yp[t * A.ny];
    }
}

// target: the moments unit's shape -- 64 pairs a block, a lane each, tiles of 64 pairs x MEAS_TILE samples of y staged through
// LDS with loads along the samples, every wave reading its lane's column -- with the chains of a pair split over
// MEAS_TARGET_WAVES waves (ROLE): 0 the error chains See, emax, Pee (carry e_prev), 1 the target chains Stt, St, Ptt (carry
// t_prev, no read of y), 2 the one mixed chain Syt; two or three dependent fp64 additions per lane and sample.  The phase s is
// formed once per lane and chunk in 64-bit integers and advanced by compare-and-wrap.  A UNIFORM wave (wuni: its pairs share
// which, row and lag) takes the tile's 64 target values once, lane l that of sample l, and broadcasts the current one
// (acme_meas_bcast: no memory access); any other wave gathers per lane, eight samples' loads ahead of the chains.  The values
// and the order of every chain are meas_target_chain's.
template <int ROLE>
__device__ inline void acme_meas_target_step(double y, double t, double c, double &a0, double &a1, double &a2, double &pv) {
    ACME_NO_CONTRACT
    using namespace acme;
    if (ROLE == 0) {
        const double e = y - t;
        const double ee = e * e;
        a0 = a0 + ee;
        a1 = meas_max(a1, fabs(e));
        const double ce = c * pv;
        const double de = e - ce;
        const double dee = de * de;
        a2 = a2 + dee;
        pv = e;
    } else if (ROLE == 1) {
        const double tt = t * t;
        a0 = a0 + tt;
        a1 = a1 + t;
        const double ct = c * pv;
        const double dt = t - ct;
        const double dtt = dt * dt;
        a2 = a2 + dtt;
        pv = t;
    } else {
        const double yt = y * t;
        a0 = a0 + yt;
    }
}
// one tile of nt samples: trow the lane's row of the y tile, tg the target row, s the phase of the tile's first sample (of the
// lane's pair; uniform: of the wave's), advanced to the next tile's
template <int ROLE>
__device__ inline void acme_meas_target_tile(const double *trow, int nt, bool uni, const double *tg, long long &s, long long P,
                                             double c, int lane, double &a0, double &a1, double &a2, double &pv) {
    using namespace acme;
    if (uni) {
        long long q = s + lane;                         // (s < P, lane < 64)
        if (P >= 64) { if (q >= P) q -= P; } else q = (long long)((int)q % (int)P);
        const double tl = lane < nt ? tg[q] : 0.0;     // lane t holds sample t's target
        if (nt == MEAS_TILE) {                          // (a whole tile: a fixed trip count the compiler unrolls)
#pragma unroll 8
            for (int t = 0; t < MEAS_TILE; ++t)
                acme_meas_target_step<ROLE>(ROLE == 1 ? 0.0 : trow[t], acme_meas_bcast(tl, t), c, a0, a1, a2, pv);
        } else {
            for (int t = 0; t < nt; ++t)
                acme_meas_target_step<ROLE>(ROLE == 1 ? 0.0 : trow[t], acme_meas_bcast(tl, t), c, a0, a1, a2, pv);
        }
        s += nt;
        if (P >= 64) { if (s >= P) s -= P; } else s = (long long)((int)s % (int)P);
        return;
    }
    int t = 0;
    for (; t + 8 <= nt; t += 8) {
        double tv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {                  // the eight loads are in flight together
            tv[k] = tg[s];
            if (++s == P) s = 0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) acme_meas_target_step<ROLE>(ROLE == 1 ? 0.0 : trow[t + k], tv[k], c, a0, a1, a2, pv);
    }
    for (; t < nt; ++t) {
        const double tv = tg[s];
        if (++s == P) s = 0;
        acme_meas_target_step<ROLE>(ROLE == 1 ? 0.0 : trow[t], tv, c, a0, a1, a2, pv);
    }
}
__global__ __launch_bounds__(64 * acme::MEAS_TARGET_WAVES) void acme_meas_target_kernel(acme::MeasTargetArgs A) {
    using namespace acme;
    __shared__ double tile[64][MEAS_TILE + 1];          // [pair][sample]: column reads by lane hit distinct banks
    __shared__ long long base[64];                      // a pair's first element of the chunk in y
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const long long Pn = A.n * A.nrows, p0 = (long long)blockIdx.x * 64, p = p0 + lane;
    const bool mine = p < Pn;
    const bool uni = A.wuni[blockIdx.x] != 0;           // (wave-uniform: one value per block)
    const long long pq = uni || !mine ? p0 : p;         // the pair whose target row and phase the lane walks (p0 < Pn)
    const long long i = pq / A.nrows, j = pq - i * A.nrows;
    if (threadIdx.x < 64 && mine) {
        const long long ip = p / A.nrows;
        base[lane] = (ip * A.pitch + A.t0) * A.ny + A.row[p - ip * A.nrows];
    }
    const double *tg = A.tgt + ((long long)A.which[i] * A.nrows + j) * A.P;
    long long s = (A.m0 % A.P + A.lag[i]) % A.P;        // once per lane and chunk, in 64-bit integers
    // the role's planes: 0 -- See, emax, Pee, e_prev; 1 -- Stt, St, Ptt, t_prev; 2 -- Syt
    const int i0 = role == 0 ? 0 : role == 1 ? 1 : 2, i1 = role == 0 ? 4 : 3, i2 = role == 0 ? 5 : 6, i3 = role == 0 ? 7 : 8;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, pv = 0.0;
    if (mine && A.m0 != 0) {                            // (the window's first sample starts from 0.0 without reading)
        a0 = A.acc[i0 * Pn + p];
        if (role < 2) { a1 = A.acc[i1 * Pn + p]; a2 = A.acc[i2 * Pn + p]; pv = A.acc[i3 * Pn + p]; }
    }
    for (long long tb = 0; tb < A.len; tb += MEAS_TILE) {
        const int nt = (int)(A.len - tb < MEAS_TILE ? A.len - tb : MEAS_TILE);
        __syncthreads();                                // (the previous tile has been read by every wave)
        for (int pp = role; pp < 64; pp += MEAS_TARGET_WAVES)   // wave pp: pair pp's samples, one per lane
            if (p0 + pp < Pn && lane < nt) tile[pp][lane] = A.y[base[pp] + (tb + lane) * A.ny];
        __syncthreads();
        if (role == 0) acme_meas_target_tile<0>(tile[lane], nt, uni, tg, s, A.P, A.c, lane, a0, a1, a2, pv);
        else if (role == 1) acme_meas_target_tile<1>(tile[lane], nt, uni, tg, s, A.P, A.c, lane, a0, a1, a2, pv);
        else acme_meas_target_tile<2>(tile[lane], nt, uni, tg, s, A.P, A.c, lane, a0, a1, a2, pv);
    }
    if (mine) {
        A.acc[i0 * Pn + p] = a0;
        if (role < 2) { A.acc[i1 * Pn + p] = a1; A.acc[i2 * Pn + p] = a2; A.acc[i3 * Pn + p] = pv; }
    }
}

// weighting: 64 pairs a block, a lane each, tiles of 64 pairs x MEAS_TILE samples.  The MEAS_WEIGHT_WAVES waves stage
// jointly: wave q loads, writes to LDS and stores the SAME sixteen pairs' rows (loads and stores along the samples), so a
// buffer's reuse by its rows' owner is ordered inside that wave and ONE barrier per tile is enough -- tile k + 1's loads are
// issued, wave 0 walks tile k's chains in place in its buffer (a lane per pair, a column of the padded tile; the sections of the
// cascade unrolled in the lane, S a template argument so that the states are registers), the loaded rows go to the other
// buffer, barrier, every wave stores its rows of tile k.  The values and their order are meas_weight_chain's.
template <int S>
__global__ __launch_bounds__(64 * acme::MEAS_WEIGHT_WAVES) void acme_meas_weight_kernel(acme::MeasWeightArgs A) {
    using namespace acme;
    constexpr int PW = 64 / MEAS_WEIGHT_WAVES;          // pairs a wave stages
    __shared__ double tile[2][64][MEAS_TILE + 1];       // [buffer][pair][sample]: column reads by lane hit distinct banks
    __shared__ long long base[64], wbase[64];           // a pair's first element of the slice in y and in w
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long Pn = A.n * A.nrows, p0 = (long long)blockIdx.x * 64, p = p0 + lane;
    const bool mine = p < Pn, chain = wave == 0 && mine;
    if (threadIdx.x < 64 && mine) {
        const long long ip = p / A.nrows, j = p - ip * A.nrows;
        base[lane] = ip * A.pitch * A.ny + A.row[j];
        wbase[lane] = ip * A.len * A.nrows + j;
    }
    double c[S][5];                                     // the coefficients in vector registers: 10 S scalar ones do not fit
#pragma unroll
    for (int k = 0; k < S; ++k) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double v = A.sos[k][q];
            asm volatile("" : "+v"(v));
            c[k][q] = v;
        }
    }
    double s1[S], s2[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        s1[k] = chain ? A.state[2 * k * Pn + p] : 0.0;
        s2[k] = chain ? A.state[(2 * k + 1) * Pn + p] : 0.0;
    }
    __syncthreads();
    const int npair = (int)(Pn - p0 < 64 ? Pn - p0 : 64);       // the block's pairs
    double r[PW];
#pragma unroll
    for (int q = 0; q < PW; ++q) {                      // tile 0
        const int pp = wave * PW + q;
        r[q] = pp < npair && lane < A.len ? A.y[base[pp] + (long long)lane * A.ny] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < PW; ++q) tile[0][wave * PW + q][lane] = r[q];
    __syncthreads();
    int buf = 0;
    for (long long tb = 0; tb < A.len; tb += MEAS_TILE, buf ^= 1) {
        const int nt = (int)(A.len - tb < MEAS_TILE ? A.len - tb : MEAS_TILE);
        const long long tn = tb + MEAS_TILE;            // the next tile's first sample
        const bool more = tn < A.len;
        if (more) {                                     // its loads are in flight during this tile's chains
#pragma unroll
            for (int q = 0; q < PW; ++q) {
                const int pp = wave * PW + q;
                r[q] = pp < npair && tn + lane < A.len ? A.y[base[pp] + (tn + lane) * A.ny] : 0.0;
            }
        }
        if (chain) {
            double *trow = tile[buf][lane];
            if (nt == MEAS_TILE) {                      // (a whole tile: a fixed trip count the compiler unrolls)
#pragma unroll 8
                for (int t = 0; t < MEAS_TILE; ++t) {
                    double x = trow[t];
#pragma unroll
                    for (int k = 0; k < S; ++k) x = meas_weight_section(c[k], x, s1[k], s2[k]);
                    trow[t] = x;
                }
            } else {
                for (int t = 0; t < nt; ++t) {
                    double x = trow[t];
#pragma unroll
                    for (int k = 0; k < S; ++k) x = meas_weight_section(c[k], x, s1[k], s2[k]);
                    trow[t] = x;
                }
            }
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < PW; ++q) tile[buf ^ 1][wave * PW + q][lane] = r[q];
        }
        __syncthreads();                                // (this tile's chains are done, the next tile is in LDS)
#pragma unroll
        for (int q = 0; q < PW; ++q) {
            const int pp = wave * PW + q;
            if (pp < npair && lane < nt) A.w[wbase[pp] + (tb + lane) * A.nrows] = tile[buf][pp][lane];
        }
    }
    if (chain) {
#pragma unroll
        for (int k = 0; k < S; ++k) { A.state[2 * k * Pn + p] = s1[k]; A.state[(2 * k + 1) * Pn + p] = s2[k]; }
    }
}

// ensemble: a lane per recorded slot of the chunk, walking the member list of its (group, row) pair in order -- the list's
// entries are wave-uniform (scalar loads), a member's load is the lanes' samples of that instance (at ny = 1 and stride = 1
// 64 consecutive doubles), MEAS_ENS_AHEAD members' loads are issued before the first of their chain steps.  ROLE 0 ... 3: the
// one chain S | Q | min | max (SPLIT: the four waves of a block share a tile of 64 slots); ROLE 4: all four (the four
// waves of a block take four tiles).  No LDS, no barrier: a lane without a slot leaves at once.  The values and the order of
// every chain are meas_ensemble_chain's.
template <int ROLE>
__device__ inline void acme_meas_ens_step(double v, long long i, double &S, double &Q, double &mn, double &mx, long long &imin,
                                          long long &imax) {
    using namespace acme;
    if (ROLE == 0 || ROLE == 4) meas_ens_sum(S, v);
    if (ROLE == 1 || ROLE == 4) meas_ens_sq(Q, v);
    if (ROLE == 2 || ROLE == 4) meas_ens_min(mn, imin, v, i);
    if (ROLE == 3 || ROLE == 4) meas_ens_max(mx, imax, v, i);
}
template <int ROLE>
__device__ inline void acme_meas_ens_walk(const acme::MeasEnsArgs &A, long long gr, long long e) {
    using namespace acme;
    const long long GR = (long long)A.G * A.nrows, g = gr / A.nrows, j = gr - g * A.nrows;
    const double *yp = A.y + (A.t0 + (e * A.stride - A.m0)) * A.ny + A.row[j];
    const long long ipitch = A.pitch * A.ny, k1 = A.off[g + 1];
    double S = 0.0, Q = 0.0, mn = INFINITY, mx = -INFINITY;
    long long imin = -1, imax = -1, k = A.off[g];
    for (; k + MEAS_ENS_AHEAD <= k1; k += MEAS_ENS_AHEAD) {
        int id[MEAS_ENS_AHEAD];
        double v[MEAS_ENS_AHEAD];
#pragma unroll
        for (int q = 0; q < MEAS_ENS_AHEAD; ++q) {      // the loads are in flight together
            id[q] = A.member[k + q];
            v[q] = yp[(long long)id[q] * ipitch];
        }
#pragma unroll
        for (int q = 0; q < MEAS_ENS_AHEAD; ++q) acme_meas_ens_step<ROLE>(v[q], id[q], S, Q, mn, mx, imin, imax);
    }
    for (; k < k1; ++k) {
        const long long i = A.member[k];
        acme_meas_ens_step<ROLE>(yp[i * ipitch], i, S, Q, mn, mx, imin, imax);
    }
    const long long at = gr * A.E + e, plane = GR * A.E;
    if (ROLE == 0 || ROLE == 4) A.acc[at] = S;
    if (ROLE == 1 || ROLE == 4) A.acc[plane + at] = Q;
    if (ROLE == 2 || ROLE == 4) { A.acc[2 * plane + at] = mn; A.arg[at] = imin; }
    if (ROLE == 3 || ROLE == 4) { A.acc[3 * plane + at] = mx; A.arg[plane + at] = imax; }
}
// grid: (group, row) pairs x the blocks of a pair's slots -- tiles of 64 (SPLIT) or of 64 * MEAS_ENS_WAVES slots
template <bool SPLIT>
__global__ __launch_bounds__(64 * acme::MEAS_ENS_WAVES) void acme_meas_ensemble_kernel(acme::MeasEnsArgs A) {
    using namespace acme;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long per = SPLIT ? 64 : 64 * MEAS_ENS_WAVES, blocks = (A.nrec + per - 1) / per;
    const long long gr = (long long)blockIdx.x / blocks, tb = (long long)blockIdx.x - gr * blocks;
    const long long q = tb * per + (SPLIT ? 0 : 64 * wave) + lane;     // the lane's slot of the chunk
    if (q >= A.nrec) return;
    const long long e = A.e0 + q;
    if (!SPLIT) acme_meas_ens_walk<4>(A, gr, e);
    else if (wave == 0) acme_meas_ens_walk<0>(A, gr, e);
    else if (wave == 1) acme_meas_ens_walk<1>(A, gr, e);
    else if (wave == 2) acme_meas_ens_walk<2>(A, gr, e);
    else acme_meas_ens_walk<3>(A, gr, e);
}
__global__ __launch_bounds__(256) void acme_meas_ens_start_kernel(double *acc, long long *arg, long long plane) {
    const long long at = (long long)blockIdx.x * 256 + threadIdx.x;
    if (at < plane) acme::meas_ens_start(acc, arg, plane, at);
}

// histogram: ONE WAVE PER PAIR (the range, the scale and the pair's addresses are wave-uniform), `waves` pairs a block.  The
// wave's lanes stride over the chunk's samples, MEAS_HIST_AHEAD loads each in flight; a sample's counter (meas_hist_bin) goes
// up by LDS integer atomic add in the wave's own B + 3 counters of 32 bits (a chunk is at most MEAS_CHUNK samples); the lanes
// then add the non-zero ones into the pair's 64-bit counters in global memory with plain load / add / store -- nobody else
// owns the pair.  AGG: neighbouring lanes hold neighbouring samples, so on a constant or slowly moving signal they hit ONE
// counter and the atomics serialise; the first lane of each run of equal counters among neighbouring lanes (one DPP shift, one
// ballot) adds the run's length instead.  Counts are integers: both shapes give the same result.
__device__ inline void acme_meas_hist_add_runs(unsigned int *h, int k, int lane) {
    const int prev = __builtin_amdgcn_update_dpp(k, k, 0x138, 0xf, 0xf, false);     // wave_shr:1 (lane 0 keeps its own)
    const bool head = lane == 0 || prev != k;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);       // the heads above this lane
    const int run = above ? __builtin_ctzll(above) + 1 : 64 - lane;
    if (head && k >= 0) atomicAdd(&h[k], (unsigned int)run);
}
template <bool AGG>
__global__ __launch_bounds__(64 * acme::MEAS_HIST_WAVES) void acme_meas_hist_kernel(acme::MeasHistArgs A, int waves) {
    using namespace acme;
    extern __shared__ unsigned int acme_meas_hist_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), C = A.B + 3;
    const long long p = (long long)blockIdx.x * waves + wave;
    const bool live = p < A.n * A.nrows;                // (wave-uniform; every wave of the block reaches both barriers)
    unsigned int *h = acme_meas_hist_lds + wave * C;
    for (int c = lane; c < C; c += 64) h[c] = 0u;
    __syncthreads();
    if (live) {
        const long long i = p / A.nrows;
        const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
        const double lo = A.range[3 * i], hi = A.range[3 * i + 1], s = A.range[3 * i + 2];
        const bool rect = A.mode == MEAS_HIST_ABS;
        for (long long tb = 0; tb < A.len; tb += 64 * MEAS_HIST_AHEAD) {
            double v[MEAS_HIST_AHEAD];
            bool on[MEAS_HIST_AHEAD];
#pragma unroll
            for (int u = 0; u < MEAS_HIST_AHEAD; ++u) {     // the loads are in flight together
                const long long t = tb + 64 * u + lane;
                on[u] = t < A.len;
                v[u] = on[u] ? yp[t * A.ny] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < MEAS_HIST_AHEAD; ++u) {
                const int k = on[u] ? meas_hist_bin(rect ? fabs(v[u]) : v[u], lo, hi, s, A.B) : -1;
                if (AGG) acme_meas_hist_add_runs(h, k, lane);
                else if (k >= 0) atomicAdd(&h[k], 1u);
            }
        }
    }
    __syncthreads();
    if (live) {
        long long *g = A.cnt + p * C;
        for (int c = lane; c < C; c += 64) {
            const unsigned int n = h[c];
            if (n) g[c] += (long long)n;
        }
    }
}

// events: ONE WAVE PER PAIR, MEAS_EVENTS_WAVES pairs a block; no LDS, no atomic, no barrier -- nobody else owns the pair.  The
// chunk is walked in ROUNDS of 64 consecutive samples, lane l holding sample 64 j + l (a wave's load is 512 contiguous bytes at
// ny = 1), MEAS_EVENTS_AHEAD rounds' loads in flight.  The loaded value stays in its register while the C levels are walked:
// per level two compares straight into scalar masks (S1: v >= hi, S0: v <= lo and not S1, both inside the round's valid
// lanes) and meas_events_masks, 64-bit scalar arithmetic -- not one floating-point operation beyond the comparisons.  What
// belongs to LEVEL c lives in LANE c's registers and is read with v_readlane and written under lane == c, the lane index the
// loop's counter: a loop over a run-time C with no register array indexed by it.  Per level THREE packed words: `pk`, the
// state in bits 0 ... 1 with the chunk's HIGH count from bit 2 and its LOW count from bit 17 (a chunk has at most 16 383
// samples: the launcher refuses more); `ev`, the chunk's rises | falls << 16; `at`, the chunk sample of the last rise |
// that of the last fall << 16 (0xffff: none).  A round without an event -- most -- costs the level two compares, five lane
// reads and one select.  In a round with events the event lanes write their own slots while the direction has room
// (the ordinal: the events so far + v_mbcnt of the mask below the lane), v[m - 1] being the lane below (DPP wave_shr:1, lane
// 0 taking the previous round's last value or the carried one).  The last event of a direction is only a POSITION until the
// chunk's end; lane c then reads its two values back from y (the chunk's first sample has the carried value below it) and
// stores the last-event slot, the counters, the state and, lane 0, the last value with plain vector stores.
__device__ inline double acme_meas_ev_readlane(double x, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}
__device__ inline double acme_meas_ev_below(double v, double first) {      // the lane below's v; lane 0: `first`
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(first), __double2loint(v), 0x138, 0xf, 0xf, false);    // wave_shr:1
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(first), __double2hiint(v), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__global__ __launch_bounds__(64 * acme::MEAS_EVENTS_WAVES) void acme_meas_events_kernel(acme::MeasEventsArgs A) {
    using namespace acme;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), C = A.C, E = A.E;
    const long long p = (long long)blockIdx.x * MEAS_EVENTS_WAVES + wave;
    if (p >= A.n * A.nrows) return;                     // (wave-uniform)
    const long long i = p / A.nrows;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    const bool mine = lane < C;                         // lane c keeps level c
    const long long q = p * C + (mine ? lane : 0);
    long long *cq = A.cnt + q * 5, *iq = A.idx + q * 2 * (E + 1);
    double *aq = A.ab + q * 4 * (E + 1);
    double lo = 0.0, hi = 0.0;
    long long base[2] = {0, 0};
    int pk = MEAS_EV_UNKNOWN, ev = 0, at = -1, room = 0;    // room: the free slots at the chunk's start, rises | falls << 16
    if (mine) {
        lo = A.lev[lane * A.n + i];
        hi = A.lev[(C + lane) * A.n + i];
        pk = A.state[q];
        base[0] = cq[0];
        base[1] = cq[1];
        room = (base[0] < E ? E - (int)base[0] : 0) | (base[1] < E ? E - (int)base[1] : 0) << 16;
    }
    const double carried0 = A.prev[p];
    double carried = carried0;
    for (long long tb = 0; tb < A.len; tb += 64 * MEAS_EVENTS_AHEAD) {
        double v[MEAS_EVENTS_AHEAD];
#pragma unroll
        for (int u = 0; u < MEAS_EVENTS_AHEAD; ++u) {   // the loads are in flight together
            const long long t = tb + 64 * u + lane;
            v[u] = t < A.len ? yp[t * A.ny] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < MEAS_EVENTS_AHEAD; ++u) {
            const int r0 = (int)tb + 64 * u;
            if (r0 < A.len) {                           // (wave-uniform)
                const int nv = A.len - r0 < 64 ? (int)(A.len - r0) : 64;
                const unsigned long long valid = nv == 64 ? ~0ull : (1ull << nv) - 1;
                for (int c = 0; c < C; ++c) {
                    const double l = acme_meas_ev_readlane(lo, c), h = acme_meas_ev_readlane(hi, c);
                    const unsigned long long S1 = __builtin_amdgcn_ballot_w64(v[u] >= h) & valid;
                    const unsigned long long S0 = __builtin_amdgcn_ballot_w64(v[u] <= l) & valid & ~S1;
                    const int w = __builtin_amdgcn_readlane(pk, c);
                    const MeasEventsMasks K = meas_events_masks(S0, S1, w & 3, valid);
                    const bool me = lane == c;
                    pk = me ? (w & ~3) + (__builtin_popcountll(K.high) << 2) + (__builtin_popcountll(K.low) << 17) + K.carry : pk;
                    if (K.rise | K.fall) {              // (wave-uniform; most rounds have no event)
                        const int done = __builtin_amdgcn_readlane(ev, c), rm = __builtin_amdgcn_readlane(room, c);
                        int where = __builtin_amdgcn_readlane(at, c);
#pragma unroll
                        for (int d = 0; d < 2; ++d) {
                            const unsigned long long M = d ? K.fall : K.rise;
                            if (!M) continue;
                            const int dn = done >> 16 * d & 0xffff, free_ = rm >> 16 * d & 0xffff;
                            if (dn < free_) {           // the direction has room: the event lanes write their slots
                                const double a = acme_meas_ev_below(v[u], carried);
                                const int ord = dn + (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(M >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)M, 0u));
                                if ((M >> lane & 1) && ord < free_) {
                                    const long long rec = ((p * C + c) * 2 + d) * (E + 1);
                                    meas_events_slot(A.idx + rec, A.ab + rec * 2, E, (long long)(E - free_) + ord, A.m0 + r0 + lane, a, v[u]);
                                }
                            }
                            const int top = r0 + 63 - __builtin_clzll(M);   // the round's last event of the direction
                            where = d ? (where & 0xffff) | top << 16 : (where & ~0xffff) | top;
                        }
                        at = me ? where : at;
                        ev = me ? done + __builtin_popcountll(K.rise) + (__builtin_popcountll(K.fall) << 16) : ev;
                    }
                }
                carried = acme_meas_ev_readlane(v[u], nv - 1);
            }
        }
    }
    if (mine) {
        const long long nh = pk >> 2 & 0x7fff, nl = pk >> 17 & 0x7fff;
        cq[0] = base[0] + (ev & 0xffff);
        cq[1] = base[1] + (ev >> 16 & 0xffff);
        cq[2] += nh;
        cq[3] += nl;
        cq[4] += A.len - nh - nl;
        A.state[q] = pk & 3;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            const int t = at >> 16 * d & 0xffff;
            if (t != 0xffff) {                          // the direction's last event of the chunk: its two values, read back
                iq[d * (E + 1) + E] = A.m0 + t;
                aq[(d * (E + 1) + E) * 2] = t ? yp[(long long)(t - 1) * A.ny] : carried0;
                aq[(d * (E + 1) + E) * 2 + 1] = yp[(long long)t * A.ny];
            }
        }
    }
    if (lane == 0) A.prev[p] = carried;
}
namespace acme {
inline int meas_events_launch(const MeasEventsArgs &A, hipStream_t st) {
    const long long pairs = A.n * A.nrows;
    if (pairs <= 0 || A.len <= 0) return 0;
    if (A.len > 16383) return (int)hipErrorInvalidValue;    // (the kernel's packed words; a chunk is MEAS_CHUNK at most)
    const unsigned blocks = (unsigned)((pairs + MEAS_EVENTS_WAVES - 1) / MEAS_EVENTS_WAVES);
    hipLaunchKernelGGL(acme_meas_events_kernel, dim3(blocks), dim3(64 * MEAS_EVENTS_WAVES), 0, st, A);
    return (int)hipGetLastError();
}
// counters 0, slots (-1, 0.0, 0.0), states UNKNOWN, the last values 0.0
inline int meas_events_zero(long long *cnt, long long *idx, double *ab, int *state, double *prev, size_t pairs, int C, int E) {
    const size_t tri = pairs * (size_t)C, rec = tri * 2 * (size_t)(E + 1);
    if (!tri) return 0;
    int rc = (int)hipMemset(cnt, 0, sizeof(long long) * tri * 5);
    if (!rc) rc = (int)hipMemset(idx, 0xff, sizeof(long long) * rec);
    if (!rc) rc = (int)hipMemset(ab, 0, sizeof(double) * rec * 2);
    if (!rc) rc = (int)hipMemset(state, 0, sizeof(int) * tri);
    if (!rc) rc = (int)hipMemset(prev, 0, sizeof(double) * pairs);
    return rc;
}
// the pairs of a block: as many waves as keep the block's counters within MEAS_HIST_LDS bytes, MEAS_HIST_WAVES at most
inline int meas_hist_waves(int B) {
    const int w = MEAS_HIST_LDS / ((B + 3) * (int)sizeof(unsigned int));
    return w < 1 ? 1 : w > MEAS_HIST_WAVES ? MEAS_HIST_WAVES : w;
}
// the runs of equal counters aggregated before the atomic unless ACME_HIST_AGG=0 in the environment (A/B measurements, tests)
inline bool meas_hist_agg() {
    const char *e = getenv("ACME_HIST_AGG");
    return !(e && e[0] == '0');
}
inline int meas_hist_launch(const MeasHistArgs &A, hipStream_t st) {
    const long long pairs = A.n * A.nrows;
    if (pairs <= 0 || A.len <= 0) return 0;
    const int w = meas_hist_waves(A.B);
    const unsigned blocks = (unsigned)((pairs + w - 1) / w);
    const size_t lds = sizeof(unsigned int) * (size_t)w * (size_t)(A.B + 3);
    if (meas_hist_agg()) hipLaunchKernelGGL(acme_meas_hist_kernel<true>, dim3(blocks), dim3(64 * w), lds, st, A, w);
    else hipLaunchKernelGGL(acme_meas_hist_kernel<false>, dim3(blocks), dim3(64 * w), lds, st, A, w);
    return (int)hipGetLastError();
}
inline int meas_hist_zero(long long *cnt, size_t count) { return count ? (int)hipMemset(cnt, 0, sizeof(long long) * count) : 0; }
// SPLIT where the unsplit launch would leave SIMDs without a wave; ACME_ENS_SPLIT=0 / 1 in the environment forces one (A/B
// measurements, tests)
inline bool meas_ens_split(long long pairs, long long nrec) {
    if (const char *e = getenv("ACME_ENS_SPLIT")) { if (e[0] == '0') return false; if (e[0] == '1') return true; }
    return pairs * ((nrec + 63) / 64) < MEAS_ENS_SPLIT_BELOW;
}
inline int meas_ensemble_launch(const MeasEnsArgs &A, hipStream_t st) {
    const long long pairs = (long long)A.G * A.nrows;
    if (pairs <= 0 || A.nrec <= 0) return 0;
    if (meas_ens_split(pairs, A.nrec))
        hipLaunchKernelGGL(acme_meas_ensemble_kernel<true>, dim3((unsigned)(pairs * ((A.nrec + 63) / 64))), dim3(64 * MEAS_ENS_WAVES), 0, st, A);
    else
        hipLaunchKernelGGL(acme_meas_ensemble_kernel<false>, dim3((unsigned)(pairs * ((A.nrec + 64 * MEAS_ENS_WAVES - 1) / (64 * MEAS_ENS_WAVES)))),
                           dim3(64 * MEAS_ENS_WAVES), 0, st, A);
    return (int)hipGetLastError();
}
// every slot back to the start values (plane = G nrows E elements)
inline int meas_ensemble_start(double *acc, long long *arg, size_t plane) {
    if (plane == 0) return 0;
    hipLaunchKernelGGL(acme_meas_ens_start_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, 0, acc, arg, (long long)plane);
    return (int)hipGetLastError();
}
template <int S>
inline int meas_weight_launch_s(const MeasWeightArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(acme_meas_weight_kernel<S>, dim3((unsigned)((A.n * A.nrows + 63) / 64)), dim3(64 * MEAS_WEIGHT_WAVES), 0, st, A);
    return (int)hipGetLastError();
}
inline int meas_weight_launch(const MeasWeightArgs &A, hipStream_t st) {
    if (A.n * A.nrows <= 0 || A.len <= 0) return 0;
    switch (A.S) {
    case 1: return meas_weight_launch_s<1>(A, st);
    case 2: return meas_weight_launch_s<2>(A, st);
    case 3: return meas_weight_launch_s<3>(A, st);
    case 4: return meas_weight_launch_s<4>(A, st);
    case 5: return meas_weight_launch_s<5>(A, st);
    case 6: return meas_weight_launch_s<6>(A, st);
    case 7: return meas_weight_launch_s<7>(A, st);
    case 8: return meas_weight_launch_s<8>(A, st);
    }
    return (int)hipErrorInvalidValue;
}
inline int meas_weight_zero(double *p, size_t count) { return (int)hipMemset(p, 0, sizeof(double) * count); }
inline int meas_target_launch(const MeasTargetArgs &A, hipStream_t st) {
    const long long pairs = A.n * A.nrows;
    if (pairs <= 0) return 0;
    hipLaunchKernelGGL(acme_meas_target_kernel, dim3((unsigned)((pairs + 63) / 64)), dim3(64 * MEAS_TARGET_WAVES), 0, st, A);
    return (int)hipGetLastError();
}
inline int meas_target_zero(double *p, size_t count) { return (int)hipMemset(p, 0, sizeof(double) * count); }
template <int LOG2L>
inline int meas_cross_launch_l(const MeasCrossArgs &C, hipStream_t st) {
    if constexpr (LOG2L > 12) {
        return (int)hipErrorInvalidValue;
    } else {
        if ((1ll << LOG2L) != C.S.L) return meas_cross_launch_l<LOG2L + 1>(C, st);
        hipLaunchKernelGGL(acme_meas_cross_kernel<LOG2L>, dim3((unsigned)(C.S.n * C.S.nrows)), dim3(256), 0, st, C);
        return (int)hipGetLastError();
    }
}
inline int meas_cross_launch(const MeasCrossArgs &C, hipStream_t st) {
    return C.S.n * C.S.nrows > 0 ? meas_cross_launch_l<6>(C, st) : 0;
}
inline int meas_cross_zero(double *p, size_t count) { return (int)hipMemset(p, 0, sizeof(double) * count); }
template <int LOG2L>
inline int meas_spectrum_launch_l(const MeasSpecArgs &A, hipStream_t st) {
    if constexpr (LOG2L > 12) {
        return (int)hipErrorInvalidValue;
    } else {
        if ((1ll << LOG2L) != A.L) return meas_spectrum_launch_l<LOG2L + 1>(A, st);
        hipLaunchKernelGGL(acme_meas_spectrum_kernel<LOG2L>, dim3((unsigned)(A.n * A.nrows)), dim3(256), 0, st, A);
        return (int)hipGetLastError();
    }
}
inline int meas_spectrum_launch(const MeasSpecArgs &A, hipStream_t st) {
    return A.n * A.nrows > 0 ? meas_spectrum_launch_l<6>(A, st) : 0;
}
inline int meas_spectrum_zero(double *p, size_t count) { return (int)hipMemset(p, 0, sizeof(double) * count); }
inline int meas_fold_launch(const MeasFoldArgs &A, hipStream_t st) {
    const long long pairs = A.n * A.nrows;
    hipLaunchKernelGGL(acme_meas_fold_kernel, dim3((unsigned)((pairs + MEAS_FOLD_WAVES - 1) / MEAS_FOLD_WAVES)),
                       dim3(64 * MEAS_FOLD_WAVES), 0, st, A);
    return (int)hipGetLastError();
}
inline int meas_fold_zero(double *fold, size_t count) { return (int)hipMemset(fold, 0, sizeof(double) * count); }
inline int meas_launch(const MeasTwArgs &T, const MeasArgs &A, hipStream_t st) {
    if (A.H > 0) {
        hipLaunchKernelGGL(acme_meas_tw_kernel, dim3((unsigned)((A.H * A.len + 255) / 256)), dim3(256), 0, st, T);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    int waves = 1, groups = 1;
    meas_shape(A.H, &waves, &groups);
    const long long P = A.n * A.nrows;
    hipLaunchKernelGGL(acme_meas_kernel, dim3((unsigned)((P + 63) / 64), (unsigned)groups), dim3(64 * waves), 0, st, A);
    return (int)hipGetLastError();
}
// the per-instance kernel on a table that is written: shared by the per-instance form and the bins
inline int meas_pi_run(const MeasPiArgs &B, hipStream_t st) {
    const MeasArgs &A = B.A;
    int waves = 1, groups = 1;
    meas_shape(A.H, &waves, &groups);
    const long long P = A.n * A.nrows;
    hipLaunchKernelGGL(acme_meas_pi_kernel, dim3((unsigned)((P + 63) / 64), (unsigned)groups), dim3(64 * waves), 0, st, B);
    return (int)hipGetLastError();
}
inline int meas_pi_launch(const MeasPiTwArgs &T, const MeasPiArgs &B, hipStream_t st) {
    const MeasArgs &A = B.A;
    if (A.H > 0) {
        const long long total = (long long)T.F * A.H * A.len;
        hipLaunchKernelGGL(acme_meas_pi_tw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, T);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    return meas_pi_run(B, st);
}
// bins: the table from the groups' reduced bins, then the per-instance kernel with H = B
inline int meas_bins_launch(const MeasBinsTwArgs &T, const MeasPiArgs &B, hipStream_t st) {
    const MeasArgs &A = B.A;
    if (A.H > 0) {
        const long long total = (long long)T.F * A.H * A.len;
        hipLaunchKernelGGL(acme_meas_bins_tw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, T);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    return meas_pi_run(B, st);
}
// series: the chunk's table (any form), then the one series kernel
inline int meas_series_launch(const MeasSeriesTwArgs &T, const MeasSeriesArgs &G, bool pi, hipStream_t st) {
    const MeasArgs &A = G.B.A;
    if (A.H > 0) {
        const long long total = (long long)T.F * A.H * A.len;
        hipLaunchKernelGGL(acme_meas_series_tw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, T);
        const int e = (int)hipGetLastError();
        if (e) return e;
    }
    int waves = 1, groups = 1;
    meas_shape(A.H, &waves, &groups);
    const long long P = A.n * A.nrows;
    const dim3 grid((unsigned)((P + 63) / 64), (unsigned)groups), block(64 * waves);
    if (pi) hipLaunchKernelGGL(acme_meas_series_kernel<true>, grid, block, 0, st, G);
    else hipLaunchKernelGGL(acme_meas_series_kernel<false>, grid, block, 0, st, G);
    return (int)hipGetLastError();
}
}  // namespace acme
#else
namespace acme {
// spectrum: the contract's arithmetic literally, pair by pair, segment by segment, stage by stage
ACME_NO_CONTRACT_FN inline void meas_spectrum_chain(const MeasSpecArgs &A, long long p) {
    ACME_NO_CONTRACT
    const long long i = p / A.nrows, L = A.L;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    double *carry = A.carry + p * L, *acc = A.acc + p * (L / 2 + 1);
    long long s_lo, s_hi;
    meas_spec_segments(A.m0, A.len, L, A.hop, &s_lo, &s_hi);
    int bits = 0;
    while ((1ll << bits) < L) ++bits;
    std::vector<double> vr((size_t)L), vi((size_t)L);
    for (long long s = s_lo; s <= s_hi; ++s) {
        for (long long j = 0; j < L; ++j) {
            const long long m = s * A.hop + j;
            long long r = 0;
            for (int k = 0; k < bits; ++k) r |= (j >> k & 1) << (bits - 1 - k);
            vr[(size_t)r] = A.w[j] * (m >= A.m0 ? yp[(m - A.m0) * A.ny] : carry[m & (L - 1)]);
            vi[(size_t)r] = 0.0;
        }
        for (long long h = 1; h < L; h *= 2)
            for (long long i0 = 0; i0 < L; ++i0) {
                if (i0 & h) continue;
                const long long k = (i0 & (h - 1)) * (L / (2 * h));
                const double wr = A.tw[2 * k], wi = A.tw[2 * k + 1], br = vr[(size_t)(i0 + h)], bi = vi[(size_t)(i0 + h)];
                const double p0 = wr * br, p1 = wi * bi, p2 = wr * bi, p3 = wi * br;
                const double tr = p0 - p1, ti = p2 + p3;
                vr[(size_t)(i0 + h)] = vr[(size_t)i0] - tr;
                vi[(size_t)(i0 + h)] = vi[(size_t)i0] - ti;
                vr[(size_t)i0] = vr[(size_t)i0] + tr;
                vi[(size_t)i0] = vi[(size_t)i0] + ti;
            }
        for (long long k = 0; k <= L / 2; ++k) {
            const double pr = vr[(size_t)k] * vr[(size_t)k], pi = vi[(size_t)k] * vi[(size_t)k];
            const double pw = pr + pi;
            acc[k] = acc[k] + pw;
        }
    }
    for (long long t = A.len > L ? A.len - L : 0; t < A.len; ++t) carry[(A.m0 + t) & (L - 1)] = yp[t * A.ny];
}
inline int meas_spectrum_launch(const MeasSpecArgs &A, void *) {
    for (long long p = 0; p < A.n * A.nrows; ++p) meas_spectrum_chain(A, p);
    return 0;
}
inline int meas_spectrum_zero(double *p, size_t count) {
    std::fill(p, p + count, 0.0);
    return 0;
}
// cross-spectrum: the contract's arithmetic literally, pair by pair, segment by segment, stage by stage
ACME_NO_CONTRACT_FN inline void meas_cross_chain(const MeasCrossArgs &C, long long p) {
    ACME_NO_CONTRACT
    const MeasSpecArgs &A = C.S;
    const long long i = p / A.nrows, L = A.L, NK = L / 2 + 1;
    const double *yp = A.y + (i * A.pitch + A.t0) * A.ny + A.row[p - i * A.nrows];
    const double *up = C.u + (i * C.upitch + A.t0) * C.nu + C.in_row;
    double *cx = A.carry + p * (2 * L), *cy = cx + L, *acc = A.acc + p * (4 * NK);
    long long s_lo, s_hi;
    meas_spec_segments(A.m0, A.len, L, A.hop, &s_lo, &s_hi);
    int bits = 0;
    while ((1ll << bits) < L) ++bits;
    std::vector<double> vr((size_t)L), vi((size_t)L);
    for (long long s = s_lo; s <= s_hi; ++s) {
        for (long long j = 0; j < L; ++j) {
            const long long m = s * A.hop + j;
            long long r = 0;
            for (int k = 0; k < bits; ++k) r |= (j >> k & 1) << (bits - 1 - k);
            vr[(size_t)r] = A.w[j] * (m >= A.m0 ? up[(m - A.m0) * C.nu] : cx[m & (L - 1)]);
            vi[(size_t)r] = A.w[j] * (m >= A.m0 ? yp[(m - A.m0) * A.ny] : cy[m & (L - 1)]);
        }
        for (long long h = 1; h < L; h *= 2)
            for (long long i0 = 0; i0 < L; ++i0) {
                if (i0 & h) continue;
                const long long k = (i0 & (h - 1)) * (L / (2 * h));
                const double wr = A.tw[2 * k], wi = A.tw[2 * k + 1], br = vr[(size_t)(i0 + h)], bi = vi[(size_t)(i0 + h)];
                const double p0 = wr * br, p1 = wi * bi, p2 = wr * bi, p3 = wi * br;
                const double tr = p0 - p1, ti = p2 + p3;
                vr[(size_t)(i0 + h)] = vr[(size_t)i0] - tr;
                vi[(size_t)(i0 + h)] = vi[(size_t)i0] - ti;
                vr[(size_t)i0] = vr[(size_t)i0] + tr;
                vi[(size_t)i0] = vi[(size_t)i0] + ti;
            }
        for (long long k = 0; k <= L / 2; ++k) {
            const long long n = (L - k) & (L - 1);
            const double zrk = vr[(size_t)k], zik = vi[(size_t)k], zrn = vr[(size_t)n], zin = vi[(size_t)n];
            const double xr = 0.5 * (zrk + zrn), xi = 0.5 * (zik - zin);
            const double yr = 0.5 * (zik + zin), yi = 0.5 * (zrn - zrk);
            const double q0 = xr * xr, q1 = xi * xi, q2 = yr * yr, q3 = yi * yi;
            const double q4 = xr * yr, q5 = xi * yi, q6 = xr * yi, q7 = xi * yr;
            const double sxx = q0 + q1, syy = q2 + q3, sre = q4 + q5, sim = q6 - q7;
            acc[k] = acc[k] + sxx;
            acc[NK + k] = acc[NK + k] + syy;
            acc[2 * NK + k] = acc[2 * NK + k] + sre;
            acc[3 * NK + k] = acc[3 * NK + k] + sim;
        }
    }
    for (long long t = A.len > L ? A.len - L : 0; t < A.len; ++t) {
        cx[(A.m0 + t) & (L - 1)] = up[t * C.nu];
        cy[(A.m0 + t) & (L - 1)] = yp[t * A.ny];
    }
}
inline int meas_cross_launch(const MeasCrossArgs &C, void *) {
    for (long long p = 0; p < C.S.n * C.S.nrows; ++p) meas_cross_chain(C, p);
    return 0;
}
inline int meas_cross_zero(double *p, size_t count) {
    std::fill(p, p + count, 0.0);
    return 0;
}
inline int meas_weight_launch(const MeasWeightArgs &A, void *) {
    for (long long p = 0; p < A.n * A.nrows; ++p) meas_weight_chain(A, p);
    return 0;
}
inline int meas_weight_zero(double *p, size_t count) {
    std::fill(p, p + count, 0.0);
    return 0;
}
inline int meas_target_launch(const MeasTargetArgs &A, void *) {
    for (long long p = 0; p < A.n * A.nrows; ++p) meas_target_chain(A, p);
    return 0;
}
inline int meas_target_zero(double *p, size_t count) {
    std::fill(p, p + count, 0.0);
    return 0;
}
inline int meas_ensemble_launch(const MeasEnsArgs &A, void *) {
    for (long long gr = 0; gr < (long long)A.G * A.nrows; ++gr)
        for (long long e = A.e0; e < A.e0 + A.nrec; ++e) meas_ensemble_chain(A, gr, e);
    return 0;
}
inline int meas_ensemble_start(double *acc, long long *arg, size_t plane) {
    for (size_t at = 0; at < plane; ++at) meas_ens_start(acc, arg, (long long)plane, (long long)at);
    return 0;
}
inline int meas_hist_launch(const MeasHistArgs &A, void *) {
    for (long long p = 0; p < A.n * A.nrows; ++p) meas_hist_chain(A, p);
    return 0;
}
inline int meas_hist_zero(long long *cnt, size_t count) {
    std::fill(cnt, cnt + count, 0ll);
    return 0;
}
// the contract's sequential loop unless ACME_EVENTS_WALK=mask in the environment: then the rounds of 64 through the mask
// algebra the device kernel runs (an unsupported test hook, like ACME_HIST_AGG)
inline int meas_events_launch(const MeasEventsArgs &A, void *) {
    const char *e = getenv("ACME_EVENTS_WALK");
    const bool mask = e && e[0] == 'm';
    for (long long p = 0; p < A.n * A.nrows; ++p) {
        if (mask) meas_events_mask_walk(A, p);
        else meas_events_chain(A, p);
    }
    return 0;
}
inline int meas_events_zero(long long *cnt, long long *idx, double *ab, int *state, double *prev, size_t pairs, int C, int E) {
    const size_t tri = pairs * (size_t)C, rec = tri * 2 * (size_t)(E + 1);
    std::fill(cnt, cnt + tri * 5, 0ll);
    std::fill(idx, idx + rec, -1ll);
    std::fill(ab, ab + rec * 2, 0.0);
    std::fill(state, state + tri, (int)MEAS_EV_UNKNOWN);
    std::fill(prev, prev + pairs, 0.0);
    return 0;
}
inline int meas_fold_launch(const MeasFoldArgs &A, void *) {
    for (long long p = 0; p < A.n * A.nrows; ++p) meas_fold_chain(A, p);
    return 0;
}
inline int meas_fold_zero(double *fold, size_t count) {
    std::fill(fold, fold + count, 0.0);
    return 0;
}
inline int meas_launch(const MeasTwArgs &T, const MeasArgs &A, void *) {
    for (long long idx = 0; idx < A.H * A.len; ++idx) meas_tw(T, idx);
    for (long long p = 0; p < A.n * A.nrows; ++p)
        for (int u = 0; u <= A.H; ++u) meas_chain(A, p, u);
    return 0;
}
// slot by slot through the plan, every unit's chain on the table row of the slot's group
inline int meas_pi_run(const MeasPiArgs &B) {
    for (long long q = 0; q < B.A.n * B.A.nrows; ++q) {
        MeasArgs A = B.A;
        A.tw = B.A.tw + 2 * (long long)B.sgrp[q] * A.H * A.len;
        for (int u = 0; u <= A.H; ++u) meas_chain(A, B.perm[q], u);
    }
    return 0;
}
inline int meas_pi_launch(const MeasPiTwArgs &T, const MeasPiArgs &B, void *) {
    for (long long idx = 0; idx < (long long)T.F * B.A.H * B.A.len; ++idx) meas_pi_tw(T, idx);
    return meas_pi_run(B);
}
inline int meas_bins_launch(const MeasBinsTwArgs &T, const MeasPiArgs &B, void *) {
    for (long long idx = 0; idx < (long long)T.F * B.A.H * B.A.len; ++idx) meas_bins_tw(T, idx);
    return meas_pi_run(B);
}
inline int meas_series_launch(const MeasSeriesTwArgs &T, const MeasSeriesArgs &G, bool pi, void *) {
    const MeasArgs &A = G.B.A;
    for (long long idx = 0; idx < (long long)T.F * A.H * A.len; ++idx) meas_series_tw(T, idx);
    for (long long q = 0; q < A.n * A.nrows; ++q) {
        const double *twg = A.tw + (pi ? 2 * (long long)G.B.sgrp[q] * A.H * A.len : 0);
        for (int u = 0; u <= A.H; ++u) meas_series_chain(A, G.S, twg, pi ? G.B.perm[q] : q, u);
    }
    return 0;
}
}  // namespace acme
#endif
