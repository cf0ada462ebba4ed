// acme_source.h -- input signals generated on the device (acme_batch_set_source_*): an input row with a source needs no
// u from the caller -- its value at clock n (base-rate samples since the first source was armed) for instance i is
//
//   CONST   offset_i
//   SINE    fma(amp_i, sin(th), offset_i),  th = 2 pi kappa / f_den,  kappa = (f_num_i n + phase_i) mod f_den taken to
//           (-f_den / 2, f_den / 2]: the phase reduced exactly in 64-bit integers, the angle formed as meas_twiddle forms
//           it (phase_angle, acme_measure.h)
//   TABLE   fma(amp_i, w[n mod P], offset_i)
//   MULTISINE  a sum of 1 ... SRC_MAX_TONES sines as ONE chain in tone order: v = offset_i, then v = fma(amp_ki, sin(th_k), v)
//           for k = 0 ... tones - 1, each th_k reduced and formed as SINE's from f_num_ki, phase_ki (per-tone arrays [tones][N]);
//           one tone is the SINE row bit for bit
//   NOISE   counter based: one Philox4x32-10 block per (instance, row, q = n div hold) -- counter (q mod 2^32, q div 2^32,
//           row, 0), key (stream_i mod 2^32, stream_i div 2^32) -- gives r0 ... r3 and the 53-bit draw
//           x = r0 + 2^32 (r1 mod 2^21);
//           UNIFORM   fma(amp_i, U, offset_i),  U = (2 x + 1 - 2^53) 2^-53 (exact, odd: in (-1, 1), never 0)
//           GAUSSIAN  fma(amp_i, g, offset_i),  g = sqrt(-2 log(u1)) sin(th),  u1 = (x + 1) 2^-53,  th = phase_angle(r2, 2^32)
//           a sample depends on (stream_i, row, q) alone: never on the slice, tile, thread or call that computes it
//   PULSE   fma(amp_i, e, offset_i) with e the instance's trapezoid envelope: five integers per instance -- period P_i
//           (1 ... 2^31 - 1), delay_i (0 ... P_i - 1), rise_i, on_i, fall_i >= 0 with rise + on + fall <= P_i -- and
//           j = (n - delay_i) mod P_i, reduced exactly in 64-bit integers (n mod P_i first):
//             e = (double)j / (double)rise                         j < rise
//                 1.0                                              rise <= j < rise + on
//                 (double)(rise + on + fall - j) / (double)fall    rise + on <= j < rise + on + fall
//                 0.0                                              otherwise
//           every integer is below 2^31, so the conversions are exact and a ramp sample is ONE correctly rounded division;
//           with the final fma two roundings at most.  rise = fall = 0: high for exactly `on` samples per period (duty on / P)
//   BURST   g = amp_i e (one rounded product, always formed), then fma(g, sin(th), offset_i) with th SINE's angle from
//           (f_num_i n + phase_i) mod f_den: the SINE row bit for bit where e = 1, offset_i where e = 0.  The tone runs with the
//           CLOCK, it does not restart per burst: a burst starts at a zero crossing of the tone when delay and P are multiples
//           of the tone's period.  (The sine is evaluated where e = 0 too: the value is the same.)
//           On an oversampled batch an ideal edge (rise = 0 or fall = 0) wants its row HELD (held_rows): the interpolator
//           would ring on it
//
// One launch per time slice (acme_api.inc run_os, where the expand kernel sits for constant rows) writes the slice's full
// [N][len][nu] block: sourced rows generated, the others gathered from the caller's rows.
//
// A block takes SRC_INST instances x one tile of SRC_TILE samples; per instance the tile's (sample, row) elements are
// contiguous, and the threads walk them side by side: a thread keeps ONE row (two neighbouring elements where 16-byte
// stores are possible: rows r, r + 1 of a sample when nu is even, samples t, t + 1 when nu = 1) and steps dt samples per
// iteration, so a wave's store is one contiguous run.  What depends on the row only (the clock reduced mod f_den / P, the
// step dt mod f_den) is computed once per thread; per instance a thread reads its row's parameters once and reduces
// kappa = (f_num_i m0 + phase_i) mod f_den and the step (f_num_i dt) mod f_den exactly (operands below 2^31: products
// below 2^62); from there kappa += step with one conditional subtraction per sample -- the integers are exact, so every
// sample's kappa is the closed form's.  Table rows: the tile's window of w (min(tile, P) entries, the same for every
// instance) is staged in LDS once per block while the rows' windows fit SRC_LDS doubles; rows beyond that read w from
// HBM / L2.  A MULTISINE row keeps one kappa and one step PER TONE (the same two reductions per tone and instance, the same
// conditional subtraction per tone and sample); a launch with such a row takes the kernel's second instantiation
// (src_thread<SRC_MODE_MULTI>, acme_source_multi_kernel: src_plan decides), a launch with a NOISE row the third
// (src_thread<SRC_MODE_NOISE>, acme_source_noise_kernel: the first kernel's kinds and NOISE), a launch with NOISE and MULTISINE
// rows the fourth (src_thread<SRC_MODE_NOISE_MULTI>, acme_source_noise_multi_kernel), every other launch the one it always
// took.  A NOISE row keeps q and n mod hold of the thread's first sample (the row's and the thread's alone) and steps
// them by dt div hold, dt mod hold with one conditional carry: no division per sample; only the key is the instance's.
// A PULSE or BURST row keeps, per instance, j of the thread's first sample and the step dt mod P_i (the two reductions, where
// SINE has its two), then j += step with one conditional subtraction per sample; j, the step, P and the thresholds rise,
// rise + on, rise + on + fall are 32-bit values.  A launch with such a row and otherwise the first kernel's kinds takes the fifth
// instantiation (src_thread<SRC_MODE_PULSE>, acme_source_pulse_kernel), one that also holds MULTISINE or NOISE rows the sixth,
// which has every kind (src_thread<SRC_MODE_ALL>, acme_source_all_kernel); launches without such a row take exactly the four
// kernels above.  In both, a SINE row is rendered as the BURST row of e = 1 (g = amp_i 1.0 = amp_i: the same bits).
//
// The per-thread functions are host + device code; the launchers below are __global__ launches under hipcc and plain
// loops over (block, thread) otherwise (the CPU emulator of tests/emu compiles acme_api.inc, and with it this file, with
// g++): both run the same index arithmetic.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "acme_common.h"
#include "acme_measure.h"

namespace acme {

constexpr int SRC_NONE = 0, SRC_CONST = 1, SRC_SINE = 2, SRC_TABLE = 3, SRC_MULTISINE = 4, SRC_NOISE = 5;      // (include/acme_hip.h: ACME_SOURCE_*)
constexpr int SRC_PULSE = 6, SRC_BURST = 7;
constexpr int SRC_UNIFORM = 0, SRC_GAUSSIAN = 1;    // a NOISE row's distribution (ACME_NOISE_*)
// the source kernel's instantiations (src_plan): bit 0: the launch may hold MULTISINE rows; bit 1: NOISE rows; bit 2: PULSE
// or BURST rows (alone, or with both other bits: the instantiation of every kind)
constexpr int SRC_MODE_PLAIN = 0, SRC_MODE_MULTI = 1, SRC_MODE_NOISE = 2, SRC_MODE_NOISE_MULTI = 3, SRC_MODE_PULSE = 4, SRC_MODE_ALL = 7;
constexpr double SRC_2M53 = 1.0 / 9007199254740992.0;      // 2^-53: the scale of a NOISE row's 53-bit draw
constexpr int SRC_MAX_TONES = 4;            // tones of a MULTISINE row (ACME_MAX_SOURCE_TONES)
constexpr long long SRC_MAX_TABLE = 1ll << 24;
constexpr int SRC_BLOCK = 256;              // threads per block
constexpr int SRC_TILE = 4096;              // samples per block
constexpr int SRC_INST = 4;                 // instances per block
constexpr int SRC_LDS = 4096;               // doubles of LDS for the table rows' windows (32 KB)

// one input row (an array of 64 in device memory; the per-instance arrays [n], NULL = the default for every instance)
struct alignas(128) SrcRow {        // (a power of two apart: a row is addressed by a shift, as it was at 64 bytes)
    int kind;                   // SRC_*; SRC_NONE: the caller's row
    int var;                    // SRC_NONE: the row's place among the caller's rows
    long long den;              // SINE, MULTISINE: f_den; TABLE: P; NOISE: hold
    const double *amp, *off;    // default 1, 0
    const long long *fnum, *phase;      // default 0, 0; NOISE: fnum holds the streams (default: stream_i = i)
    const double *w;            // TABLE: [P]
    int tones;                  // MULTISINE: amp, fnum, phase are [tones][n] (tone k of instance i at [k * n + i]); NOISE: SRC_UNIFORM / _GAUSSIAN
    const long long *shape;     // PULSE, BURST: [5][n] -- period, delay, rise, on, fall (entry k of instance i at [k * n + i])
};

struct SrcArgs {
    double *dst;                // instance i, sample t, row r at dst[(i * dpitch + t) * nu + r]
    const double *uv;           // the caller's rows: uv[(i * upitch + t) * nin + v]; NULL: zeros
    const SrcRow *rows;         // [nu] (nu <= 64)
    long long n, len, dpitch, upitch;
    long long n0;               // the clock at the slice's first sample
    int nu, nin;
    int vec;                    // 16-byte stores: nu even, or nu = 1 with len and dpitch even; dst 16-byte aligned
    unsigned long long lds_rows;        // the table rows whose windows are staged in LDS
    int mode;                   // SRC_MODE_*: the instantiation the launch takes (src_plan)
};

struct alignas(16) SrcPair { double a, b; };

// the first entry of w a tile needs: (n0 + tb) mod P
ACME_HD inline unsigned long long src_table_base(const SrcArgs &A, long long P, long long tb) {
    return ((unsigned long long)(A.n0 % P) + (unsigned long long)tb) % (unsigned long long)P;
}
// a table row's window in LDS: offset (the windows of the staged rows before it) and length for a tile of tl samples
ACME_HD inline int src_lds_offset(const SrcArgs &A, int row) {
    const long long tmax = A.len < SRC_TILE ? A.len : SRC_TILE;
    long long off = 0;
    for (int r = 0; r < row; ++r)
        if (A.lds_rows >> r & 1ull) off += A.rows[r].den < tmax ? A.rows[r].den : tmax;
    return (int)off;
}

// the block's windows: lds[off + q] = w[(base + q) mod P], q < min(tl, P)
ACME_HD inline void src_stage(const SrcArgs &A, long long by, int tid, double *lds) {
    const long long tb = by * SRC_TILE, tl = A.len - tb < SRC_TILE ? A.len - tb : SRC_TILE;
    for (int r = 0; r < A.nu; ++r) {
        if (!(A.lds_rows >> r & 1ull)) continue;
        const SrcRow &R = A.rows[r];
        const long long P = R.den, win = P < tl ? P : tl;
        const long long base = (long long)src_table_base(A, P, tb);
        double *o = lds + src_lds_offset(A, r);
        for (long long q = tid; q < win; q += SRC_BLOCK) {
            const long long j = base + q;                   // < 2 P
            o[q] = R.w[j >= P ? j - P : j];
        }
    }
}

// what a thread keeps of one of its rows: everything that does not depend on the instance ...
struct SrcSlot {
    int kind, var, tones;
    unsigned long long den;     // SINE, MULTISINE: f_den; TABLE: the index's modulus (the window's length, or P from HBM)
    unsigned long long m0;      // SINE: (n0 + first sample) mod f_den; TABLE: the first sample's index
    unsigned long long dstep;   // dt mod den
    const double *amp, *off, *tab;
    const long long *fnum, *phase;
};
// ... and the instance's: parameters, the running phase / index and its step
struct SrcRun {
    double amp, off;
    unsigned long long k, step;
    const double *u;            // SRC_NONE: the caller's row at the thread's next sample
};
// a MULTISINE row's tones 1 ... SRC_MAX_TONES - 1 beside tone 0 (which lives in amp, k, step above)
struct SrcRunMulti : SrcRun {
    double ampx[SRC_MAX_TONES - 1];
    unsigned long long kx[SRC_MAX_TONES - 1], stepx[SRC_MAX_TONES - 1];
};
// a NOISE row beside those: the row's counter at the thread's first sample and its step (n mod hold and dt mod hold live in
// m0 and dstep above, hold in den) ...
struct SrcSlotNoise : SrcSlot {
    unsigned long long q0, dq;  // (n0 + first sample) div hold; dt div hold
    unsigned int row;           // the counter's third word
};
// ... and the instance's key; the running counter (n mod hold runs in k above); Base: SrcRun, or SrcRunMulti in a launch that
// holds MULTISINE rows too
template <class Base> struct SrcRunNoise : Base {
    unsigned long long q;
    unsigned int key0, key1;
};
// a PULSE or BURST row beside those: the integer block, and what the per-instance reductions need of the thread ...
template <class Base> struct SrcSlotPulse : Base {
    const long long *shape;
    unsigned long long first;   // the thread's first sample within the slice
    unsigned int dt;            // samples per step
};
// ... and the instance's envelope: the running j, its step, the period and the thresholds rise, rise + on, rise + on + fall
template <class Base> struct SrcRunPulse : Base {
    unsigned int j, jstep, per, t1, t2, t3;
};
template <int MODE> struct SrcRunOf { typedef SrcRun type; };
template <> struct SrcRunOf<SRC_MODE_MULTI> { typedef SrcRunMulti type; };
template <> struct SrcRunOf<SRC_MODE_NOISE> { typedef SrcRunNoise<SrcRun> type; };
template <> struct SrcRunOf<SRC_MODE_NOISE_MULTI> { typedef SrcRunNoise<SrcRunMulti> type; };
template <> struct SrcRunOf<SRC_MODE_PULSE> { typedef SrcRunPulse<SrcRun> type; };
template <> struct SrcRunOf<SRC_MODE_ALL> { typedef SrcRunPulse<SrcRunNoise<SrcRunMulti> > type; };
template <int MODE> struct SrcSlotOf { typedef SrcSlot type; };
template <> struct SrcSlotOf<SRC_MODE_NOISE> { typedef SrcSlotNoise type; };
template <> struct SrcSlotOf<SRC_MODE_NOISE_MULTI> { typedef SrcSlotNoise type; };
template <> struct SrcSlotOf<SRC_MODE_PULSE> { typedef SrcSlotPulse<SrcSlot> type; };
template <> struct SrcSlotOf<SRC_MODE_ALL> { typedef SrcSlotPulse<SrcSlotNoise> type; };

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants): counter c, key k -> four words
struct SrcWords { unsigned int r0, r1, r2, r3; };
ACME_HD inline SrcWords src_philox(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0, unsigned int k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned int)p1; c3 = (unsigned int)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return SrcWords{c0, c1, c2, c3};
}
// a NOISE row's draw from its block's words, before amp and offset: U or g (the operations in exactly this order)
ACME_HD inline double src_noise_draw(const SrcWords &w, int dist) {
    const unsigned long long x = (unsigned long long)w.r0 + ((unsigned long long)(w.r1 & 0x1FFFFFu) << 32);       // 53 bits
    if (dist == SRC_UNIFORM) return (double)((long long)(2ull * x + 1ull) - (1ll << 53)) * SRC_2M53;       // (an odd integer below 2^53: exact)
    const double u1 = (double)(x + 1ull) * SRC_2M53;         // (0, 1], exact
    const double th = phase_angle((long long)w.r2, 1ll << 32);
    const double rad = sqrt(-2.0 * log(u1));
    return rad * sin(th);
}

// row `row`, first sample tb + ts of the slice, dt samples per step (MODE: the launch may hold MULTISINE rows)
template <int MODE>
ACME_HD inline void src_slot_init(const SrcArgs &A, int row, long long tb, long long tl, long long ts, long long dt, const double *lds,
                                  SrcSlot &S) {
    const SrcRow &R = A.rows[row];
    S.kind = R.kind; S.var = R.var; S.tones = R.tones;
    S.amp = R.amp; S.off = R.off; S.fnum = R.fnum; S.phase = R.phase; S.tab = R.w;
    S.den = 1; S.m0 = 0; S.dstep = 0;
    if (R.kind == SRC_SINE || ((MODE & SRC_MODE_MULTI) && R.kind == SRC_MULTISINE) || ((MODE & SRC_MODE_PULSE) && R.kind == SRC_BURST)) {
        S.den = (unsigned long long)R.den;
        S.m0 = ((unsigned long long)(A.n0 % R.den) + (unsigned long long)(tb + ts)) % S.den;      // (n mod f_den first)
        S.dstep = (unsigned long long)dt % S.den;
    } else if (R.kind == SRC_TABLE) {
        if (A.lds_rows >> row & 1ull) {
            S.den = (unsigned long long)(R.den < tl ? R.den : tl);
            S.m0 = (unsigned long long)ts % S.den;
            S.tab = lds + src_lds_offset(A, row);
        } else {
            S.den = (unsigned long long)R.den;
            S.m0 = (src_table_base(A, R.den, tb) + (unsigned long long)ts) % S.den;
        }
        S.dstep = (unsigned long long)dt % S.den;
    }
}

// ... of a launch that may hold NOISE rows: the counter and n mod hold of the thread's first sample, their steps
template <int MODE>
ACME_HD inline void src_slot_init(const SrcArgs &A, int row, long long tb, long long tl, long long ts, long long dt, const double *lds,
                                  SrcSlotNoise &S) {
    src_slot_init<MODE>(A, row, tb, tl, ts, dt, lds, static_cast<SrcSlot &>(S));
    S.q0 = 0ull; S.dq = 0ull; S.row = (unsigned int)row;
    if (S.kind != SRC_NOISE) return;
    const unsigned long long hold = (unsigned long long)A.rows[row].den, n = (unsigned long long)A.n0 + (unsigned long long)(tb + ts);
    S.den = hold;
    S.q0 = n / hold; S.m0 = n % hold;
    S.dq = (unsigned long long)dt / hold; S.dstep = (unsigned long long)dt % hold;
}

// ... of a launch that may hold PULSE or BURST rows
template <int MODE, class Base>
ACME_HD inline void src_slot_init(const SrcArgs &A, int row, long long tb, long long tl, long long ts, long long dt, const double *lds,
                                  SrcSlotPulse<Base> &S) {
    src_slot_init<MODE>(A, row, tb, tl, ts, dt, lds, static_cast<Base &>(S));
    S.shape = A.rows[row].shape;
    S.first = (unsigned long long)(tb + ts);
    S.dt = (unsigned int)dt;
}

ACME_HD inline void src_run_init(const SrcArgs &A, const SrcSlot &S, long long i, long long tb, long long ts, SrcRun &R) {
    R.amp = S.amp ? S.amp[i] : 1.0;
    R.off = S.off ? S.off[i] : 0.0;
    R.k = S.m0;
    R.step = S.dstep;
    R.u = nullptr;
    if (S.kind == SRC_SINE) {
        const unsigned long long f = S.fnum ? (unsigned long long)S.fnum[i] : 0ull, p = S.phase ? (unsigned long long)S.phase[i] : 0ull;
        R.k = (f * S.m0 + p) % S.den;               // f, m0, p < f_den < 2^31
        R.step = (f * S.dstep) % S.den;
    } else if (S.kind == SRC_NONE && A.uv)
        R.u = A.uv + (i * A.upitch + tb + ts) * A.nin + S.var;
}
// ... of a launch that may hold MULTISINE rows: per tone the two reductions of a SINE row
ACME_HD inline void src_run_init(const SrcArgs &A, const SrcSlot &S, long long i, long long tb, long long ts, SrcRunMulti &R) {
    src_run_init(A, S, i, tb, ts, static_cast<SrcRun &>(R));
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < SRC_MAX_TONES - 1; ++j) { R.ampx[j] = 0.0; R.kx[j] = 0ull; R.stepx[j] = 0ull; }
    if (S.kind != SRC_MULTISINE) return;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < SRC_MAX_TONES; ++k) {
        if (k >= S.tones) continue;         // (constant indices after unrolling: the tones stay in registers)
        const long long e = k * A.n + i;
        const unsigned long long f = (unsigned long long)S.fnum[e], p = S.phase ? (unsigned long long)S.phase[e] : 0ull;
        const unsigned long long kap = (f * S.m0 + p) % S.den, st = (f * S.dstep) % S.den;
        const double a = S.amp ? S.amp[e] : 1.0;
        if (k == 0) { R.amp = a; R.k = kap; R.step = st; }
        else { R.ampx[k - 1] = a; R.kx[k - 1] = kap; R.stepx[k - 1] = st; }
    }
}

// ... of a launch that may hold NOISE rows: the instance's key (src_run_init above has set k = n mod hold, step = dt mod hold)
template <class Base>
ACME_HD inline void src_run_init(const SrcArgs &A, const SrcSlotNoise &S, long long i, long long tb, long long ts, SrcRunNoise<Base> &R) {
    src_run_init(A, static_cast<const SrcSlot &>(S), i, tb, ts, static_cast<Base &>(R));
    R.q = S.q0; R.key0 = 0u; R.key1 = 0u;
    if (S.kind != SRC_NOISE) return;
    const unsigned long long stream = S.fnum ? (unsigned long long)S.fnum[i] : (unsigned long long)i;
    R.key0 = (unsigned int)stream; R.key1 = (unsigned int)(stream >> 32);
}

// ... of a launch that may hold PULSE or BURST rows: j = (n - delay_i) mod P_i of the thread's first sample (n mod P_i first)
// and the step dt mod P_i; the thresholds; a BURST row's tone as a SINE row's
template <class SlotBase, class RunBase>
ACME_HD inline void src_run_init(const SrcArgs &A, const SrcSlotPulse<SlotBase> &S, long long i, long long tb, long long ts,
                                 SrcRunPulse<RunBase> &R) {
    src_run_init(A, static_cast<const SlotBase &>(S), i, tb, ts, static_cast<RunBase &>(R));
    R.j = 0u; R.jstep = 0u; R.per = 1u; R.t1 = 0u; R.t2 = 0u; R.t3 = 0u;
    if (S.kind != SRC_PULSE && S.kind != SRC_BURST) return;
    const unsigned long long P = (unsigned long long)S.shape[i], delay = (unsigned long long)S.shape[A.n + i];
    const unsigned long long m = ((unsigned long long)(A.n0 % (long long)P) + S.first) % P;         // n mod P_i
    R.per = (unsigned int)P;
    R.j = (unsigned int)(m >= delay ? m - delay : m + P - delay);
    R.jstep = S.dt % R.per;
    R.t1 = (unsigned int)S.shape[2 * A.n + i];
    R.t2 = R.t1 + (unsigned int)S.shape[3 * A.n + i];
    R.t3 = R.t2 + (unsigned int)S.shape[4 * A.n + i];
    if (S.kind == SRC_BURST) {
        const unsigned long long f = S.fnum ? (unsigned long long)S.fnum[i] : 0ull, p = S.phase ? (unsigned long long)S.phase[i] : 0ull;
        R.k = (f * S.m0 + p) % S.den;
        R.step = (f * S.dstep) % S.den;
    }
}

// the trapezoid at j: one division on the ramps (exact conversions: the integers are below 2^31), no a * b + c shape anywhere
ACME_HD inline double src_envelope(unsigned int j, unsigned int t1, unsigned int t2, unsigned int t3) {
    if (j < t1) return (double)j / (double)t1;
    if (j < t2) return 1.0;
    if (j < t3) return (double)(t3 - j) / (double)(t3 - t2);
    return 0.0;
}

// the row's value at the thread's current sample; on to the next (dt samples later)
ACME_HD inline double src_next(const SrcSlot &S, SrcRun &R, long long ustep) {
    double v;
    if (S.kind == SRC_CONST) return R.off;
    if (S.kind == SRC_NONE) {
        if (!R.u) return 0.0;
        v = *R.u;
        R.u += ustep;
        return v;
    }
    if (S.kind == SRC_SINE) v = fma(R.amp, sin(phase_angle((long long)R.k, (long long)S.den)), R.off);
    else v = fma(R.amp, S.tab[R.k], R.off);
    R.k += R.step;
    if (R.k >= S.den) R.k -= S.den;
    return v;
}
// ... of a launch that may hold MULTISINE rows: the chain over the row's tones
ACME_HD inline double src_next(const SrcSlot &S, SrcRunMulti &R, long long ustep) {
    if (S.kind != SRC_MULTISINE) return src_next(S, static_cast<SrcRun &>(R), ustep);
    double v = fma(R.amp, sin(phase_angle((long long)R.k, (long long)S.den)), R.off);
    R.k += R.step;
    if (R.k >= S.den) R.k -= S.den;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < SRC_MAX_TONES - 1; ++j) {
        if (j + 1 < S.tones) {
            v = fma(R.ampx[j], sin(phase_angle((long long)R.kx[j], (long long)S.den)), v);
            R.kx[j] += R.stepx[j];
            if (R.kx[j] >= S.den) R.kx[j] -= S.den;
        }
    }
    return v;
}
// ... of a launch that may hold NOISE rows: the block of the sample's counter
template <class Base>
ACME_HD inline double src_next(const SrcSlotNoise &S, SrcRunNoise<Base> &R, long long ustep) {
    if (S.kind != SRC_NOISE) return src_next(static_cast<const SrcSlot &>(S), static_cast<Base &>(R), ustep);
    const SrcWords w = src_philox((unsigned int)R.q, (unsigned int)(R.q >> 32), S.row, 0u, R.key0, R.key1);
    const double v = fma(R.amp, src_noise_draw(w, S.tones), R.off);
    R.k += R.step;
    R.q += S.dq;
    if (R.k >= S.den) { R.k -= S.den; ++R.q; }
    return v;
}

// ... of a launch that may hold PULSE or BURST rows; a SINE row goes the BURST row's way with e = 1 (one sine in the code)
template <class SlotBase, class RunBase>
ACME_HD inline double src_next(const SrcSlotPulse<SlotBase> &S, SrcRunPulse<RunBase> &R, long long ustep) {
    if (S.kind != SRC_PULSE && S.kind != SRC_BURST && S.kind != SRC_SINE)
        return src_next(static_cast<const SlotBase &>(S), static_cast<RunBase &>(R), ustep);
    double e = 1.0;
    if (S.kind != SRC_SINE) {
        e = src_envelope(R.j, R.t1, R.t2, R.t3);
        R.j += R.jstep;                 // (both below P_i < 2^31)
        if (R.j >= R.per) R.j -= R.per;
        if (S.kind == SRC_PULSE) return fma(R.amp, e, R.off);
    }
    const double g = R.amp * e;
    const double v = fma(g, sin(phase_angle((long long)R.k, (long long)S.den)), R.off);
    R.k += R.step;
    if (R.k >= S.den) R.k -= S.den;
    return v;
}

// thread tid of block (bx, by): instances bx SRC_INST ..., samples by SRC_TILE ...
template <int MODE>
ACME_HD inline void src_thread(const SrcArgs &A, long long bx, long long by, int tid, const double *lds) {
    const int nu = A.nu;
    const long long tb = by * SRC_TILE, tl = A.len - tb < SRC_TILE ? A.len - tb : SRC_TILE;
    // the thread's elements: row r0 (and its neighbour) of samples ts, ts + dt, ...
    int r0, r1;
    long long ts, ts1, dt;
    if (A.vec && nu == 1) {
        r0 = r1 = 0; ts = 2 * tid; ts1 = ts + 1; dt = 2 * SRC_BLOCK;
    } else {
        const int per = A.vec ? nu / 2 : nu, act = SRC_BLOCK / per * per;        // units per sample; threads in use
        if (tid >= act) return;
        r0 = A.vec ? 2 * (tid % per) : tid % per;
        r1 = r0 + 1;
        ts = ts1 = tid / per;
        dt = act / per;
    }
    typedef typename SrcSlotOf<MODE>::type Slot;
    Slot s0, s1;
    if (MODE != SRC_MODE_PLAIN) s1 = Slot{};        // (read by src_run_init's tone loop only when A.vec has filled it)
    src_slot_init<MODE>(A, r0, tb, tl, ts, dt, lds, s0);
    if (A.vec) src_slot_init<MODE>(A, r1, tb, tl, ts1, dt, lds, s1);
    const long long ustep = dt * A.nin;
    for (long long i = bx * SRC_INST; i < (bx + 1) * SRC_INST && i < A.n; ++i) {
        typename SrcRunOf<MODE>::type q0, q1;
        src_run_init(A, s0, i, tb, ts, q0);
        double *d = A.dst + (i * A.dpitch + tb) * nu;
        if (A.vec) {
            src_run_init(A, s1, i, tb, ts1, q1);
            for (long long t = ts; t < tl; t += dt) {
                const SrcPair v{src_next(s0, q0, ustep), src_next(s1, q1, ustep)};
                *reinterpret_cast<SrcPair *>(d + t * nu + r0) = v;
            }
        } else {
            for (long long t = ts; t < tl; t += dt) d[t * nu + r0] = src_next(s0, q0, ustep);
        }
    }
}

// the launch's shape: which table rows are staged in LDS (in row order while their windows fit; use_lds false: none) and
// whether 16-byte stores are possible; which instantiation runs
inline void src_plan(SrcArgs &A, const SrcRow *host_rows, bool use_lds) {
    const long long tmax = A.len < SRC_TILE ? A.len : SRC_TILE;
    long long used = 0;
    A.lds_rows = 0ull;
    A.mode = SRC_MODE_PLAIN;
    for (int r = 0; r < A.nu; ++r)
        A.mode |= host_rows[r].kind == SRC_MULTISINE ? SRC_MODE_MULTI : host_rows[r].kind == SRC_NOISE ? SRC_MODE_NOISE
                  : host_rows[r].kind == SRC_PULSE || host_rows[r].kind == SRC_BURST ? SRC_MODE_PULSE : 0;
    if (A.mode > SRC_MODE_PULSE) A.mode = SRC_MODE_ALL;         // (PULSE / BURST next to MULTISINE or NOISE rows: the kernel of every kind)
    for (int r = 0; r < A.nu && use_lds; ++r) {
        if (host_rows[r].kind != SRC_TABLE) continue;
        const long long win = host_rows[r].den < tmax ? host_rows[r].den : tmax;
        if (used + win > SRC_LDS) break;
        A.lds_rows |= 1ull << r;
        used += win;
    }
    const bool even = A.nu % 2 == 0 || (A.nu == 1 && A.len % 2 == 0 && A.dpitch % 2 == 0);
    A.vec = even && (uintptr_t)A.dst % 16 == 0 ? 1 : 0;
}

// packed outputs of a slice -> the caller's array: dst[(i * pitch + t) * rows + r] = src[(i * len + t) * rows + r]
struct SrcCopyArgs { double *dst; const double *src; long long n, len, pitch; int rows; };
ACME_HD inline void src_copy(const SrcCopyArgs &A, long long idx) {
    const long long w = A.len * A.rows, i = idx / w, e = idx - i * w;
    A.dst[i * A.pitch * A.rows + e] = A.src[idx];
}

}  // namespace acme

// ---- launchers ---------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
__global__ __launch_bounds__(acme::SRC_BLOCK) void acme_source_kernel(acme::SrcArgs A) {
    __shared__ double lds[acme::SRC_LDS];
    if (A.lds_rows) {           // (uniform over the launch)
        acme::src_stage(A, blockIdx.y, threadIdx.x, lds);
        __syncthreads();
    }
    acme::src_thread<acme::SRC_MODE_PLAIN>(A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
__global__ __launch_bounds__(acme::SRC_BLOCK) void acme_source_multi_kernel(acme::SrcArgs A) {
    __shared__ double lds[acme::SRC_LDS];
    if (A.lds_rows) {           // (uniform over the launch)
        acme::src_stage(A, blockIdx.y, threadIdx.x, lds);
        __syncthreads();
    }
    acme::src_thread<acme::SRC_MODE_MULTI>(A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
__global__ __launch_bounds__(acme::SRC_BLOCK) void acme_source_noise_kernel(acme::SrcArgs A) {
    __shared__ double lds[acme::SRC_LDS];
    if (A.lds_rows) {           // (uniform over the launch; NOISE rows use no LDS)
        acme::src_stage(A, blockIdx.y, threadIdx.x, lds);
        __syncthreads();
    }
    acme::src_thread<acme::SRC_MODE_NOISE>(A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
// (two waves per SIMD: the rows' tones and counters together would take 290 registers, 34 of them accumulation registers;
// bounded to 256 the allocator parks 54 in scratch instead -- DESIGN 2.5i)
__global__ __launch_bounds__(acme::SRC_BLOCK, 2) void acme_source_noise_multi_kernel(acme::SrcArgs A) {
    __shared__ double lds[acme::SRC_LDS];
    if (A.lds_rows) {           // (uniform over the launch)
        acme::src_stage(A, blockIdx.y, threadIdx.x, lds);
        __syncthreads();
    }
    acme::src_thread<acme::SRC_MODE_NOISE_MULTI>(A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
__global__ __launch_bounds__(acme::SRC_BLOCK) void acme_source_pulse_kernel(acme::SrcArgs A) {
    __shared__ double lds[acme::SRC_LDS];
    if (A.lds_rows) {           // (uniform over the launch; PULSE and BURST rows use no LDS)
        acme::src_stage(A, blockIdx.y, threadIdx.x, lds);
        __syncthreads();
    }
    acme::src_thread<acme::SRC_MODE_PULSE>(A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
// (every kind in one launch: two waves per SIMD as acme_source_noise_multi_kernel, and for its reason; correct for every
// combination of kinds, not measured for speed -- DESIGN 2.5q)
__global__ __launch_bounds__(acme::SRC_BLOCK, 2) void acme_source_all_kernel(acme::SrcArgs A) {
    __shared__ double lds[acme::SRC_LDS];
    if (A.lds_rows) {           // (uniform over the launch)
        acme::src_stage(A, blockIdx.y, threadIdx.x, lds);
        __syncthreads();
    }
    acme::src_thread<acme::SRC_MODE_ALL>(A, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}
__global__ __launch_bounds__(256) void acme_source_copy_kernel(acme::SrcCopyArgs A) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < A.n * A.len * A.rows) acme::src_copy(A, idx);
}
namespace acme {
inline int src_launch(const SrcArgs &A, hipStream_t st) {
    const dim3 grid((unsigned)((A.n + SRC_INST - 1) / SRC_INST), (unsigned)((A.len + SRC_TILE - 1) / SRC_TILE));
    if (A.mode == SRC_MODE_ALL) hipLaunchKernelGGL(acme_source_all_kernel, grid, dim3(SRC_BLOCK), 0, st, A);
    else if (A.mode == SRC_MODE_PULSE) hipLaunchKernelGGL(acme_source_pulse_kernel, grid, dim3(SRC_BLOCK), 0, st, A);
    else if (A.mode == SRC_MODE_NOISE_MULTI) hipLaunchKernelGGL(acme_source_noise_multi_kernel, grid, dim3(SRC_BLOCK), 0, st, A);
    else if (A.mode == SRC_MODE_NOISE) hipLaunchKernelGGL(acme_source_noise_kernel, grid, dim3(SRC_BLOCK), 0, st, A);
    else if (A.mode == SRC_MODE_MULTI) hipLaunchKernelGGL(acme_source_multi_kernel, grid, dim3(SRC_BLOCK), 0, st, A);
    else hipLaunchKernelGGL(acme_source_kernel, grid, dim3(SRC_BLOCK), 0, st, A);
    return (int)hipGetLastError();
}
inline int src_launch_copy(const SrcCopyArgs &A, hipStream_t st) {
    hipLaunchKernelGGL(acme_source_copy_kernel, dim3((unsigned)((A.n * A.len * A.rows + 255) / 256)), dim3(256), 0, st, A);
    return (int)hipGetLastError();
}
}  // namespace acme
#else
namespace acme {
inline int src_launch(const SrcArgs &A, void *) {
    std::vector<double> lds(SRC_LDS);
    for (long long by = 0; by * SRC_TILE < A.len; ++by) {
        for (int tid = 0; tid < SRC_BLOCK && A.lds_rows; ++tid) src_stage(A, by, tid, lds.data());
        for (long long bx = 0; bx * SRC_INST < A.n; ++bx)
            for (int tid = 0; tid < SRC_BLOCK; ++tid) {
                if (A.mode == SRC_MODE_ALL) src_thread<SRC_MODE_ALL>(A, bx, by, tid, lds.data());
                else if (A.mode == SRC_MODE_PULSE) src_thread<SRC_MODE_PULSE>(A, bx, by, tid, lds.data());
                else if (A.mode == SRC_MODE_NOISE_MULTI) src_thread<SRC_MODE_NOISE_MULTI>(A, bx, by, tid, lds.data());
                else if (A.mode == SRC_MODE_NOISE) src_thread<SRC_MODE_NOISE>(A, bx, by, tid, lds.data());
                else if (A.mode == SRC_MODE_MULTI) src_thread<SRC_MODE_MULTI>(A, bx, by, tid, lds.data());
                else src_thread<SRC_MODE_PLAIN>(A, bx, by, tid, lds.data());
            }
    }
    return 0;
}
inline int src_launch_copy(const SrcCopyArgs &A, void *) {
    for (long long idx = 0; idx < A.n * A.len * A.rows; ++idx) src_copy(A, idx);
    return 0;
}
}  // namespace acme
#endif
