// postchain_kernels.hip -- S-meter, AGC and demodulators for gfx950 (K4 in DESIGN.md).
//
// Replaces, per channel and per burst of band-pass output, the tail of
// CDemodulator::ProcessData (reference dsp/demodulator.cpp:182-207):
//   CSMeter::ProcessData (dsp/smeter.cpp:62-93) -> CAgc::ProcessData (dsp/agc.cpp:174-296)
//   -> C{Am,Sam,Fm,Ssb}Demod::ProcessData (dsp/amdemod.cpp:66-104, samdemod.cpp:78-158,
//   fmdemod.cpp:113-236, ssbdemod.cpp:48-60) with their CFir (dsp/fir.cpp:72-127) and CIir
//   (dsp/iir.cpp:171-201) helpers.
//
// The reference runs these as one per-sample loop full of running state.  Here one wave owns one
// channel and walks it in 1024-sample tiles staged in LDS; what is not a recurrence runs on all
// 64 lanes, linear recurrences are lane scans, the two piecewise-linear ones (AGC averagers, PLLs)
// are solved under a guess that is checked afterwards and walked sample by sample when the guess
// fails (see the comment blocks below and DESIGN.md K4).  The rate here is the decimated one
// (<= 78 kS/s per channel): the kernel is measured in cycles per sample, not against a roofline.
#include <hip/hip_runtime.h>
#include "postchain.h"
#include "ref_constants.hpp"
#include <cstdlib>
#include "launch_once.hpp"
#include "pc_scan.hpp"

namespace csdr {

constexpr double kTwoPiD = 2.0 * 3.14159265358979323846;

// ---- CFir: y[n] = sum_k h[k] x[n-k] over a ring (dsp/fir.cpp:72-127) -----------------------------
__device__ __forceinline__ float fir_real(PcFir &f, float x)
{
    int p = f.pos + 1;
    if (p >= f.ntaps) p = 0;
    f.pos = p;
    f.zreal[p] = x;
    float acc = 0.f;
    int q = p;
    for (int k = 0; k < f.ntaps; k++) {
        acc += f.coef[k] * f.zreal[q];
        if (--q < 0) q = f.ntaps - 1;
    }
    return acc;
}
__device__ __forceinline__ void fir_cpx(PcFir &f, float &re, float &im)
{
    int p = f.pos + 1;
    if (p >= f.ntaps) p = 0;
    f.pos = p;
    f.zr[p] = re; f.zi[p] = im;
    float ar = 0.f, ai = 0.f;
    int q = p;
    for (int k = 0; k < f.ntaps; k++) {
        ar += f.icoef[k] * f.zr[q];
        ai += f.qcoef[k] * f.zi[q];
        if (--q < 0) q = f.ntaps - 1;
    }
    re = ar; im = ai;
}
// ---- CIir (dsp/iir.cpp:171-201) ------------------------------------------------------------------
__device__ __forceinline__ float iir_step(const PcIir &f, float x, double &w1, double &w2)
{
    const double w0 = (double)x - f.a1 * w1 - f.a2 * w2;
    const double y = f.b0 * w0 + f.b1 * w1 + f.b2 * w2;
    w2 = w1; w1 = w0;
    return (float)y;
}
__device__ __forceinline__ float iir_a(PcIir &f, float x) { return iir_step(f, x, f.w1a, f.w2a); }
__device__ __forceinline__ float iir_b(PcIir &f, float x) { return iir_step(f, x, f.w1b, f.w2b); }

// =====================================================================================================
// One workgroup of NW waves (1 or 4) per channel, 1024-sample tiles (PT, pc_scan.hpp) staged in LDS.  Thread t owns the
// LC = 1024 / (64 NW) consecutive samples [LC t, LC t + LC) in every recurrence; element-wise work is
// strided over the workgroup.
// =====================================================================================================
constexpr int PH = PC_AGC_RING;          // longest history (AGC delay / window)
constexpr int PC_NCHUNK = (PC_AGC_RING + PT) / 16, PC_RLEVELS = 8;
constexpr int LCMAX = 16;                // samples per thread at NW = 1
constexpr int BQ_TAB = (LCMAX + 1) * 4 + LCMAX * 2;   // biquad chunk tables: M^k (k <= 16), c M^k (k < 16)
constexpr double kInvTwoPiD = 1.0 / (2.0 * 3.14159265358979323846);
constexpr int PC_PLL_WARM_MAX = 192;     // longest warm-up of the overlapped PLL walks (pll_overlap) worth running
constexpr float kNegBig = -1.0e30f;

struct PcLds {
    PcSync sy;
    alignas(16) float2 dl[PH + PT];                  // [last dly_n inputs | tile]: delay line, then the AGC output in place
    alignas(16) float mg[PH + PT];                   // [last win_n-1 log-magnitudes | tile]
    alignas(16) float pk[PT + 16];                   // sliding peak, then the log gain argument
    alignas(16) float w0[PT + PC_FIR_MAX + 17];      // [FIR history | tile] work array (audio / envelope / I)
    alignas(16) float w1[PT + PC_FIR_MAX + 17];      // second work array (theta / Q)
    alignas(16) float h0[PC_FIR_MAX + 17], h1[PC_FIR_MAX + 17]; // FIR taps of the active demodulator, reversed and zero padded:
                                                    // h[4 + r] = tap ntaps-1-r (16-byte aligned rows of four)
    alignas(16) float w2[PT + 16];       // third work array (S-meter dB, attack average, PLL phase, |hp|)
    alignas(16) float rt[PC_RLEVELS][PC_NCHUNK];   // log table over the chunk maxima of the sliding peak
    double pw_sm[LCMAX + 1], pw_dc[LCMAX + 1], pw_sq[LCMAX + 1], pw_fd[LCMAX + 1];   // powers of the averager coefficients
    double bq[BQ_TAB];                   // biquad chunk tables
    double pm[(LCMAX + 1) * 4];          // PLL transition-matrix powers
};

// the image of the AGC peaks kernel (agc_peaks_kernel)
static_assert(sizeof(float) * PC_RLEVELS * PC_NCHUNK >= 8 * 512 && sizeof(float) * (PT + 16) >= 8 * 512,
              "pll_overlap keeps one double per thread in PcLds::rt and in PcLds::w2");
struct PreLds {
    PcSync sy;
    alignas(16) float mg[PH + PT];                   // [last win_n-1 log-magnitudes | tile]
    alignas(16) float pk[PT + 16];
    alignas(16) float w2[PT + 16];
    alignas(16) float rt[PC_RLEVELS][PC_NCHUNK];
};

// the squelch kernels' image (fm_squelch_*): a quarter of PcLds, so that eight of their workgroups share a CU
struct SqLds {
    PcSync sy;
    alignas(16) float w0[PT + PC_FIR_MAX + 17];      // [FIR history | tile] audio
    alignas(16) float h0[PC_FIR_MAX + 17];           // high-pass taps, reversed and zero padded
    alignas(16) float w2[PT + 16];                   // |hp| / audio being low-passed
    double pw_sq[LCMAX + 1];
    double bq[BQ_TAB];
};

__device__ __forceinline__ double wrap_turn(double a) { return a - rint(a); }    // [-0.5, 0.5]

// An EXACTLY ZERO sample in front of a PLL (round 6).  The kernels run the loops in the phase domain -- theta = arg(x), error
// = -wrap(theta + phi) -- and a zero has no argument.  The reference (fmdemod.cpp:166-172, samdemod.cpp:83-89 / 120-126) rotates
// first, t = x (cos phi + j s sin phi), and takes atan2(t.im, t.re): for x = (+-0, +-0) the products are signed zeros, their
// sum / difference is a signed zero by IEEE 754 (a - b = -0 only for (-0) - (+0); a + b = -0 only for (-0) + (-0)), and
// atan2(+-0, +0) = +-0 but atan2(+-0, -0) = +-pi: depending on the QUADRANT of phi the loop is left alone or kicked by half a
// turn.  Zeros are not exotic: the AGC's delay line is zeros for the first 15 ms of every stream, a muted input is zeros, and
// an fp32 filter's start-up is full of them (its samples are small multiples of one quantum) -- until round 5 the kernels
// took theta = 0 there, the error -wrap(phi), and the first burst of an FM receiver fed the SAME filter output differed from
// the reference's arithmetic by up to 0.6 of full scale (tests/test_randomized_gpu.py's loop-only check).
// The tile's theta array carries a zero sample as the code 4 + signbit(re) + 2 signbit(im) (no angle is beyond 0.5 turns).
__device__ __forceinline__ float pll_theta_of(float re, float im)
{
    if (re == 0.f && im == 0.f) return 4.0f + (float)(__float_as_uint(re) >> 31) + 2.0f * (float)(__float_as_uint(im) >> 31);
    return atan2f(im, re) * 0.15915494309189535f;                  // 1 / 2 pi
}
__device__ __forceinline__ bool pll_theta_is_zero_code(float v) { return v >= 3.5f; }
// the reference's phase error (turns) on such a sample; p = phi in turns, sgn = the sign s above (FM: +1; the error is -sgn atan2)
__device__ __forceinline__ double pll_zero_err(float code, double p, double sgn)
{
    const int bits = (int)code - 4;
    const bool sxr = bits & 1, sxi = bits & 2;
    const double fr = p - floor(p);                                    // [0, 1)
    const bool sc = fr > 0.25 && fr < 0.75;                            // cos(2 pi p) < 0
    const bool ss = (fr > 0.5) != (sgn < 0.0);                         // s sin(2 pi p) negative (-0 included: -1 x (+0))
    const bool neg_re = (sc != sxr) && !(ss != sxi);                   // c xr - s xi = -0
    const bool neg_im = (sc != sxi) && (ss != sxr);                    // c xi + s xr = -0
    const double a = neg_re ? (neg_im ? -0.5 : 0.5) : 0.0;             // atan2(t.im, t.re) in turns
    return -sgn * a;
}
// One exact step of the loop (fmdemod.cpp:166-177, samdemod.cpp:83-97) in turns -- wrapping is a - rint(a) -- on the sample
// theta = v: the one-thread walks of FM and SAM and the overlapped walks (pll_overlap).  FM is the SAM form with sgn = 1.0.
__device__ __forceinline__ void pll_step(float v, double &p, double &f, double alpha, double beta, double lo, double hi, double sgn)
{
    const double err = pll_theta_is_zero_code(v) ? pll_zero_err(v, p, sgn) : -sgn * wrap_turn((double)v + sgn * p);
    f = fmin(fmax(f + beta * err, lo), hi);
    p = wrap_turn(p + f + alpha * err);
}

// The outputs a thread of the tile owns: LC consecutive ones with four waves (the FIRs below then share one register
// window of the input), the strided t + NT j otherwise.
template <int NW> __device__ __forceinline__ int pc_out_index(int t, int j)
{ return NW == 4 ? Wg<NW>::LC * t + j : t + Wg<NW>::NT * j; }

// acc[j] = sum_k tap[k] * x[i_j - k], k ascending, for this thread's outputs i_j = pc_out_index(t, j).  `arr` is the
// work array [ntaps-1 history | tile | zeros], `hr` the taps as PcLds holds them (reversed, zero padded).
// Four waves: the four outputs are consecutive, so the thread walks ONE window of the array in 16-byte reads
// (ntaps/4 + 1 of them, and as many of the taps) instead of fetching every tap's sample for every output -- the
// squelch filter alone was a fifth of an FM tile.  The products are added in the same order as the plain loop
// (padded taps contribute exact zeros), so the words do not change.
template <int NW>
__device__ __forceinline__ void fir_blk(const float *hr, int ntaps, const float *arr, int t, float (&acc)[Wg<NW>::LC])
{
    constexpr int NT = Wg<NW>::NT, NO = Wg<NW>::LC;
#pragma unroll
    for (int j = 0; j < NO; j++) acc[j] = 0.f;
    if constexpr (NW == 4) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const int Q = (ntaps + 2) / 4 + 1;                      // samples 4t .. 4t + ntaps + 2 of the array
        const f4 *v = reinterpret_cast<const f4 *>(arr) + t;
        const f4 *g = reinterpret_cast<const f4 *>(hr);
        f4 B = g[Q];
        for (int q = Q - 1; q >= 0; q--) {
            const f4 A = g[q], V = v[q];
            const float cw[7] = {A.y, A.z, A.w, B.x, B.y, B.z, B.w};     // taps r = 4q-3 .. 4q+3 (+4 in hr)
            const float sv[4] = {V.x, V.y, V.z, V.w};
#pragma unroll
            for (int e = 3; e >= 0; e--)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[j] += cw[e - j + 3] * sv[e];
            B = A;
        }
    } else {
        const float *p = arr + (ntaps - 1) + t;
#pragma unroll 3
        for (int k = 0; k < ntaps; k++) {
            const float hk = hr[4 + ntaps - 1 - k];
#pragma unroll
            for (int j = 0; j < NO; j++) acc[j] += hk * p[NT * j - k];
        }
    }
}
// keep the last `hist` (< 128) entries of [hist | n] in front for the next tile; barrier inside
template <int NW>
__device__ __forceinline__ void slide(const Wg<NW> &g, float *w, int hist, int n)
{
    float keep[2] = {0.f, 0.f};
    if (g.t < 64) for (int j = 0; j < 2; j++) { const int i = g.t + 64 * j; if (i < hist) keep[j] = w[n + i]; }
    g.sync();
    if (g.t < 64) for (int j = 0; j < 2; j++) { const int i = g.t + 64 * j; if (i < hist) w[i] = keep[j]; }
}
// the same for the AGC's rings, hist <= PH: read all, one barrier, write all -- the caller's barrier follows
template <int NW, class T>
__device__ __forceinline__ void keep_tail(const Wg<NW> &g, T *w, int hist, int n)
{
    constexpr int NT = Wg<NW>::NT;
    T keep[PH / NT];
#pragma unroll
    for (int j = 0; j < PH / NT; j++) { const int i = g.t + NT * j; if (i < hist) keep[j] = w[n + i]; }
    g.sync();
#pragma unroll
    for (int j = 0; j < PH / NT; j++) { const int i = g.t + NT * j; if (i < hist) w[i] = keep[j]; }
}
// FIR taps as PcLds holds them: reversed, four zeros in front, zeros behind
template <int NT>
__device__ __forceinline__ void stage_taps(float *h, const float *coef, int nt, int t)
{
    for (int i = t; i < PC_FIR_MAX + 17; i += NT) {
        const int k = nt - 1 - (i - 4);
        h[i] = (k >= 0 && k < nt) ? coef[k] : 0.f;
    }
}

// A channel's output row: mono floats, or pairs (stereo audio with both halves alike, or complex samples)
struct PcRow {
    float *m; float2 *s; bool stereo;
    static __device__ __forceinline__ PcRow of(const PcArgs &a, int ch)
    {
        const long orow = (long)(a.out_rows ? a.out_rows[ch] : ch) * a.out_stride;
        return {a.out + orow, reinterpret_cast<float2 *>(a.out) + orow, (a.flags & PC_STEREO) != 0};
    }
    __device__ __forceinline__ void put(long i, float y) const { if (stereo) s[i] = make_float2(y, y); else m[i] = y; }
    __device__ __forceinline__ float raw(long i) const { return stereo ? s[i].x : m[i]; }
};

// CFmDemod's squelch after a burst (fmdemod.cpp:128-151): sq = the average behind the burst; hysteresis around the threshold
__device__ __forceinline__ int squelch_decide(double sq, double thresh, int squelched)
{
    if (0 == thresh) return 1;
    if (squelched) return sq < (thresh - refc::FM_SQUELCH_HYSTERESIS) ? 0 : squelched;
    return sq >= (thresh + refc::FM_SQUELCH_HYSTERESIS) ? 1 : squelched;
}

// The burst-parallel side kernels (AGC peaks, squelch maps / apply): one workgroup per (channel, group of bpw bursts).
// Host: as few bursts per workgroup as still give every workgroup a slot in ONE round (four 256-thread workgroups per
// CU at these kernels' 88-110 registers), so that taps, tables and zeroing are paid once per slot.
static int pc_bursts_per_wg(const PcArgs &a)
{
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const long slots = 4L * (cus > 0 ? cus : 256);
    const int bpw = (int)(((long)a.channels * a.nbursts + slots - 1) / slots);
    return bpw < 1 ? 1 : bpw;
}
__host__ __device__ __forceinline__ int pc_burst_groups(int nbursts, int bpw) { return (nbursts + bpw - 1) / bpw; }
// a launch's arguments, with its slot of the workgroup trace where that is compiled in
static PcArgs pc_traced(PcArgs a)
{
#ifdef CSDR_WG_TRACE
    a.trace = wgtrace_next();
#endif
    return a;
}
struct PcBurstGroup { int ch, b0, b1; };                 // this workgroup's channel and bursts [b0, b1)
__device__ __forceinline__ PcBurstGroup pc_burst_group(int nbursts, int bpw)
{
    const int ngrp = pc_burst_groups(nbursts, bpw);
    const int ch = blockIdx.x / ngrp, b0 = (blockIdx.x % ngrp) * bpw;
    return {ch, b0, b0 + bpw < nbursts ? b0 + bpw : nbursts};
}

// Thread 0 walks src[0..n) in order, f(value, index); the next eight values are fetched from LDS
// while the current eight go through the recurrence, so no LDS latency sits on the dependent chain.
// src must be readable up to n+15.  (The fallback of the guessed solves below.)
template <class F>
__device__ __forceinline__ void seq_walk(const float *src, int n, F f)
{
    float cur[8], nxt[8];
#pragma unroll
    for (int j = 0; j < 8; j++) cur[j] = src[j];
    for (int i0 = 0; i0 < n; i0 += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) nxt[j] = src[i0 + 8 + j];
        if (i0 + 8 <= n) {
#pragma unroll
            for (int j = 0; j < 8; j++) f(cur[j], i0 + j);
        } else {
            for (int j = 0; j < 8; j++) if (i0 + j < n) f(cur[j], i0 + j);
        }
#pragma unroll
        for (int j = 0; j < 8; j++) cur[j] = nxt[j];
    }
}

// =====================================================================================================
// Constant-coefficient LINEAR recurrences (averagers, DC blockers, the biquad) are not walked sample
// by sample: a thread runs its LC consecutive samples from a zero state, the chunk-start states
// follow from a workgroup scan over the affine chunk maps (a^cnt, p_last), and the homogeneous part
// a^(j+1) * S_start is added back.  Results differ from the sequential fp64 loop by rounding only.
// =====================================================================================================
__device__ __forceinline__ void pow_table(double *tab, double a, int t)    // tab[k] = a^k, k = 0..16
{
    if (t <= LCMAX) { double p = 1.0; for (int k = 0; k < t; k++) p *= a; tab[t] = p; }
}

// s_i = a s_{i-1} + g x_i  over x[0..n), n <= 1024, s_{-1} = s0.  emit(i, x_i, s_i, s_{i-1}) for every
// sample (skipped when EMIT is false).  Returns s_{n-1} on every thread.
template <bool EMIT, int NW, class F>
__device__ __forceinline__ double lin1_scan(const Wg<NW> &g, const float *x, int n, double a, double gn, double s0,
                                            const double *apw, F emit)
{
    constexpr int LC = Wg<NW>::LC;
    const int base = g.base(), cnt = g.count(n);
    float xv[LC];
    double loc[LC], p = 0.0;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        xv[j] = j < cnt ? x[base + j] : 0.f;
        p = j < cnt ? a * p + gn * (double)xv[j] : p;
        loc[j] = p;
    }
    Aff1 m{apw[cnt], p}, tot;
    g.scan(m, tot);
    const double S = m(s0);                                          // state entering this thread's chunk
    if (EMIT) {
        double prev = S;
#pragma unroll
        for (int j = 0; j < LC; j++) {
            if (j < cnt) {
                const double sj = loc[j] + apw[j + 1] * S;
                emit(base + j, xv[j], sj, prev);
                prev = sj;
            }
        }
    }
    return tot(s0);
}

// CSMeter (smeter.cpp:62-93), final state only.  att is a plain averager (Aff1); dec obeys
// dec' = max(att', (1-da) dec + da mag): one sample is the map AffMax{1-da, da mag, att'}.
// From a thread's attack map and its maximum to the attack average entering its chunk; pk: then the maximum of the whole tile
template <int NW>
__device__ __forceinline__ double smeter_att_scan(const Wg<NW> &g, const PcSMeter &sm, Aff1 att, double &pk, double &att_end)
{
    Both<Aff1, Max> m{att, {pk}}, tot;
    g.scan(m, tot);
    pk = tot.q.v;
    att_end = tot.p(sm.att_ave);
    return m.p(sm.att_ave);
}
// ... and from the threads' decay maps, the attack average and the maximum of a tile to the meter's state behind it
template <int NW>
__device__ __forceinline__ void smeter_finish(const Wg<NW> &g, PcSMeter &sm, AffMax dec, double att_end, double pk)
{
    AffMax tot;
    g.scan(dec, tot);
    const double dec_end = tot(sm.dec_ave);
    sm.att_ave = att_end; sm.dec_ave = dec_end; sm.ave_mag = dec_end; sm.peak_mag = fmax(sm.peak_mag, pk);
}
template <int NW>
__device__ __forceinline__ void smeter_tile(const Wg<NW> &g, PcSMeter &sm, const float *db, int n, const double *apw_att)
{
    constexpr int LC = Wg<NW>::LC;
    const double aa = sm.att_a, ia = 1.0 - sm.att_a, da = sm.dec_a, id = 1.0 - sm.dec_a;
    const int base = g.base(), cnt = g.count(n);
    float xv[LC];
    double loc[LC], p = 0.0, pk = -1.0e300;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        xv[j] = j < cnt ? db[base + j] : 0.f;
        p = j < cnt ? ia * p + aa * (double)xv[j] : p;
        loc[j] = p;
        if (j < cnt) pk = fmax(pk, (double)xv[j]);
    }
    double att_end;
    const double S = smeter_att_scan(g, sm, {apw_att[cnt], p}, pk, att_end);
    AffMax dec = AffMax::identity();                                 // chunk map of the decay average
#pragma unroll
    for (int j = 0; j < LC; j++)
        if (j < cnt) dec = AffMax{id, da * (double)xv[j], loc[j] + apw_att[j + 1] * S}.after(dec);   // (updated attack average)
    smeter_finish(g, sm, dec, att_end, pk);
}

// CIir direct form II (iir.cpp:171-186) over x[0..n) in place.  State s = (w1, w2):
// s' = M s + (x, 0), y = b0 x + c . s, M = [[-a1, -a2], [1, 0]], c = (b1 - b0 a1, b2 - b0 a2).
// tab: M^k (4 doubles each, k = 0..16) then r_k = c M^k (2 doubles each, k = 0..15)
__device__ __forceinline__ void biquad_table(double *tab, const PcIir &f, int t)
{
    if (t == 0) {
        double m00 = 1.0, m01 = 0.0, m10 = 0.0, m11 = 1.0;
        const double c0 = f.b1 - f.b0 * f.a1, c1 = f.b2 - f.b0 * f.a2;
        for (int k = 0; k <= LCMAX; k++) {
            tab[4 * k] = m00; tab[4 * k + 1] = m01; tab[4 * k + 2] = m10; tab[4 * k + 3] = m11;
            if (k < LCMAX) { tab[68 + 2 * k] = c0 * m00 + c1 * m10; tab[68 + 2 * k + 1] = c0 * m01 + c1 * m11; }
            const double n00 = -f.a1 * m00 - f.a2 * m10, n01 = -f.a1 * m01 - f.a2 * m11;     // M * M^k
            m10 = m00; m11 = m01; m00 = n00; m01 = n01;
        }
    }
}
// one sample of a thread's chunk, run from a zero state (w1, w2): the output without the homogeneous part; the state
// moves only while the sample is one of the tile's (live)
__device__ __forceinline__ double biquad_chunk_step(const PcIir &f, double xv, bool live, double &w1, double &w2)
{
    const double w0 = xv - f.a1 * w1 - f.a2 * w2;
    const double y = f.b0 * w0 + f.b1 * w1 + f.b2 * w2;
    if (live) { w2 = w1; w1 = w0; }
    return y;
}
// the map of a chunk of cnt samples: M^cnt from a table of matrix powers, (v0, v1) = the chunk's zero-state response
__device__ __forceinline__ Aff2 chunk_map2(const double *tab, int cnt, double v0, double v1)
{
    return {{tab[4 * cnt], tab[4 * cnt + 1], tab[4 * cnt + 2], tab[4 * cnt + 3]}, {v0, v1}};
}
template <int NW>
__device__ __forceinline__ void biquad_scan(const Wg<NW> &g, float *x, int n, PcIir &f, const double *tab)
{
    constexpr int LC = Wg<NW>::LC;
    const int base = g.base(), cnt = g.count(n);
    double y[LC], w1 = 0.0, w2 = 0.0;
#pragma unroll
    for (int j = 0; j < LC; j++) y[j] = biquad_chunk_step(f, j < cnt ? (double)x[base + j] : 0.0, j < cnt, w1, w2);
    Aff2 m = chunk_map2(tab, cnt, w1, w2), tot;
    g.scan(m, tot);
    double S1, S2;
    m(f.w1a, f.w2a, S1, S2);
    tot(f.w1a, f.w2a, f.w1a, f.w2a);                                 // (the old state goes in by value)
#pragma unroll
    for (int j = 0; j < LC; j++)
        if (j < cnt) x[base + j] = (float)(y[j] + tab[68 + 2 * j] * S1 + tab[68 + 2 * j + 1] * S2);
}

// One-tile FM burst: the squelch average (lin1_scan without emit over sq[0..n)) and, in lockstep with it, the audio
// low-pass of the burst over x[0..n) (biquad_scan) -- speculatively: whether the burst is squelched is only known
// from the average, so the filtered samples stay in registers (y, this thread's LC consecutive ones) and the
// filter state after the burst is returned in (w1n, w2n) for the caller to commit or drop.
template <int NW>
__device__ __forceinline__ double sq_and_lowpass(const Wg<NW> &g, const float *sq, const float *x, int n, double a, double gn, double s0,
                                                 const double *apw, const PcIir &f, const double *tab, float (&y)[Wg<NW>::LC],
                                                 double &w1n, double &w2n)
{
    constexpr int LC = Wg<NW>::LC;
    const int base = g.base(), cnt = g.count(n);
    double p = 0.0, yy[LC], w1 = 0.0, w2 = 0.0;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        const float sv = j < cnt ? sq[base + j] : 0.f;
        p = j < cnt ? a * p + gn * (double)sv : p;
        yy[j] = biquad_chunk_step(f, j < cnt ? (double)x[base + j] : 0.0, j < cnt, w1, w2);
    }
    Both<Aff1, Aff2> m{{apw[cnt], p}, chunk_map2(tab, cnt, w1, w2)}, tot;
    g.scan(m, tot);
    double S1, S2;
    m.q(f.w1a, f.w2a, S1, S2);
#pragma unroll
    for (int j = 0; j < LC; j++) y[j] = (float)(yy[j] + tab[68 + 2 * j] * S1 + tab[68 + 2 * j + 1] * S2);
    tot.q(f.w1a, f.w2a, w1n, w2n);
    return tot.p(s0);
}

// CAgc's attack / decay averagers (agc.cpp:233-262):  ave += alpha (pk - ave),  alpha = rise when
// pk > ave else fall.  Piecewise linear, so: guess the selector bits, solve the then-linear
// recurrence with a scan, recompute the selectors from the solution, repeat until they reproduce
// themselves -- at that point the sequence IS the sequential one (each selector was taken against
// the true previous average).  The correct prefix grows every round; the peak moves slowly, so two
// or three rounds are typical.  Returns false after PC_AGC_ROUNDS without a fixed point (the caller
// then walks the tile sample by sample).
constexpr int PC_AGC_ROUNDS = 8;
template <int NW, class F>
__device__ __forceinline__ bool agc_ave_scan(const Wg<NW> &g, const float *pk, int n, double rise, double fall, double &ave, F emit)
{
    constexpr int LC = Wg<NW>::LC;
    const int base = g.base(), cnt = g.count(n);
    const double ave0 = ave;
    float pv[LC];
    unsigned sel = 0;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        pv[j] = j < cnt ? pk[base + j] : 0.f;
        if (j < cnt && (double)pv[j] > ave0) sel |= 1u << j;
    }
#ifdef PC_CENSUS
    for (int round = 0; round < g.cen_limit; round++) {
#else
    for (int round = 0; round < PC_AGC_ROUNDS; round++) {
#endif
        Aff1 m = Aff1::identity(), tot;
#pragma unroll
        for (int j = 0; j < LC; j++) {
            if (j < cnt) {
                const double al = (sel >> j & 1) ? rise : fall;
                m.a = m.a - al * m.a;
                m.b = m.b + al * ((double)pv[j] - m.b);
            }
        }
        g.scan(m, tot);
        double x = m(ave0);
        double val[LC];
        unsigned nsel = 0;
#pragma unroll
        for (int j = 0; j < LC; j++) {
            if (j < cnt) {
                if ((double)pv[j] > x) nsel |= 1u << j;
                const double al = (sel >> j & 1) ? rise : fall;
                x = x + al * ((double)pv[j] - x);
            }
            val[j] = x;
        }
        if (!g.any(nsel != sel)) {
#pragma unroll
            for (int j = 0; j < LC; j++) if (j < cnt) emit(base + j, val[j]);
            ave = tot(ave0);
#ifdef PC_CENSUS
            g.cen_rounds = round + 1;
#endif
            return true;
        }
        sel = nsel;
    }
    return false;
}

// Both averagers (attack, decay) of a tile in the same rounds: their scans are independent, and run in lockstep
// (Both<Aff1, Aff1>).  emit(i, attack_i, decay_i).
template <int NW, class F>
__device__ __forceinline__ bool agc_ave_scan2(const Wg<NW> &g, const float *pk, int n, double a_rise, double a_fall, double d_rise,
                                              double d_fall, double &att, double &dec, F emit)
{
    constexpr int LC = Wg<NW>::LC;
    const int base = g.base(), cnt = g.count(n);
    const double att0 = att, dec0 = dec;
    float pv[LC];
    unsigned sa = 0, sd = 0;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        pv[j] = j < cnt ? pk[base + j] : 0.f;
        if (j < cnt && (double)pv[j] > att0) sa |= 1u << j;
        if (j < cnt && (double)pv[j] > dec0) sd |= 1u << j;
    }
#ifdef PC_CENSUS
    for (int round = 0; round < g.cen_limit; round++) {
#else
    for (int round = 0; round < PC_AGC_ROUNDS; round++) {
#endif
        Both<Aff1, Aff1> m = Both<Aff1, Aff1>::identity(), tot;
#pragma unroll
        for (int j = 0; j < LC; j++) {
            if (j < cnt) {
                const double al = (sa >> j & 1) ? a_rise : a_fall, dl = (sd >> j & 1) ? d_rise : d_fall;
                m.p.a = m.p.a - al * m.p.a; m.p.b = m.p.b + al * ((double)pv[j] - m.p.b);
                m.q.a = m.q.a - dl * m.q.a; m.q.b = m.q.b + dl * ((double)pv[j] - m.q.b);
            }
        }
        g.scan(m, tot);
        double x = m.p(att0), y = m.q(dec0);
        double va[LC], vd[LC];
        unsigned na = 0, nd = 0;
#pragma unroll
        for (int j = 0; j < LC; j++) {
            if (j < cnt) {
                if ((double)pv[j] > x) na |= 1u << j;
                if ((double)pv[j] > y) nd |= 1u << j;
                const double al = (sa >> j & 1) ? a_rise : a_fall, dl = (sd >> j & 1) ? d_rise : d_fall;
                x = x + al * ((double)pv[j] - x);
                y = y + dl * ((double)pv[j] - y);
            }
            va[j] = x; vd[j] = y;
        }
        if (!g.any(na != sa || nd != sd)) {
#pragma unroll
            for (int j = 0; j < LC; j++) if (j < cnt) emit(base + j, va[j], vd[j]);
            att = tot.p(att0); dec = tot.q(dec0);
#ifdef PC_CENSUS
            g.cen_rounds = round + 1;
#endif
            return true;
        }
        sa = na; sd = nd;
    }
    return false;
}

// The second-order PLL of CFmDemod / CSamDemod (fmdemod.cpp:166-177, samdemod.cpp:83-97), in turns:
//   e = -wrap(theta_i + phi),  f += beta e (clamped to [lo, hi]),  phi += f + alpha e.
// With the input phase unwrapped (Theta_i, a prefix sum of wrapped differences) a locked loop keeps
// Theta_i + phi next to ONE integer K for a whole tile and never touches the clamp; under that
// guess e = (K - Theta_i) - phi and the loop is the constant-coefficient linear system
//   [phi; f] <- [[1-alpha-beta, 1], [-beta, 1]] [phi; f] + (alpha+beta, beta) (K - Theta_i),
// solved by a scan like the biquad.  The guess is then checked sample by sample (|e| < 1/2, f
// inside the clamp); if it holds everywhere the result is the sequential one, otherwise (cycle slip,
// acquisition, noise) the caller walks the tile.  emit(i, phi_before, f_after).
// tab: M^k, k = 0..16 (4 doubles each).  ph, fr are written only when the guess held (true).
__device__ __forceinline__ void pll_table(double *tab, double alpha, double beta, int t)
{
    if (t == 0) {
        const double a00 = 1.0 - alpha - beta, a01 = 1.0, a10 = -beta, a11 = 1.0;
        double m00 = 1.0, m01 = 0.0, m10 = 0.0, m11 = 1.0;
        for (int k = 0; k <= LCMAX; k++) {
            tab[4 * k] = m00; tab[4 * k + 1] = m01; tab[4 * k + 2] = m10; tab[4 * k + 3] = m11;
            const double n00 = a00 * m00 + a01 * m10, n01 = a00 * m01 + a01 * m11;
            const double n10 = a10 * m00 + a11 * m10, n11 = a10 * m01 + a11 * m11;
            m00 = n00; m01 = n01; m10 = n10; m11 = n11;
        }
    }
}
template <int NW, class F>
__device__ __forceinline__ bool pll_scan(const Wg<NW> &g, const float *th, int n, double alpha, double beta, double lo, double hi,
                                         double &ph, double &fr, const double *tab, F emit)
{
    constexpr int LC = Wg<NW>::LC;
    const int base = g.base(), cnt = g.count(n);
#ifdef PC_CENSUS
    if (g.cen_force & 16u) {                                          // skipped: the record still says whether the tile holds a zero code
        bool cen_zero = false;
        for (int j = 0; j < LC; j++) if (j < cnt) cen_zero = cen_zero || pll_theta_is_zero_code(th[base + j]);
        g.cen_or(1u << 20 | (g.any(cen_zero) ? 1u << 19 : 0u));
        return false;
    }
#endif
    float tv[LC];
    bool zero = false;
#pragma unroll
    for (int j = 0; j < LC; j++) { tv[j] = j < cnt ? th[base + j] : 0.f; zero = zero || pll_theta_is_zero_code(tv[j]); }
    // (an exactly zero sample has no phase: the exact walks take the tile -- decided together with the guess's own check at the
    // end: a vote of its own per tile cost a single receiver's walk 0.4 us per tile, 5 % of a C2 / C5 call)
    // unwrapped input phase relative to the first sample of the tile
    float last = tv[0];
#pragma unroll
    for (int j = 1; j < LC; j++) if (j < cnt) last = tv[j];
    const float first = th[0];
    const float before = g.prev_thread(last, first);
    double c[LC], run = 0.0;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        // (the difference in fp64: in fp32 it is rounded across the half-turn wrap, |d| near 1 being one bit coarser than the
        // angles, and every wrap left up to 2^-25 turns in the unwrapped phase until the next tile dropped them as one step)
        const double d = (double)tv[j] - (double)(j == 0 ? before : tv[j - 1]);
        if (j < cnt) run += d - rint(d);
        c[j] = run;
    }
    const double ex = g.scan_sum_excl(run);
    const double K = rint((double)first + ph);
    const double off = K - (double)first - ex;
#pragma unroll
    for (int j = 0; j < LC; j++) c[j] = off - c[j];                  // K - Theta_i
    // zero-state chunk response
    double v[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < LC; j++) {
        if (j < cnt) {
            const double e = c[j] - v[0];
            v[1] = v[1] + beta * e;
            v[0] = v[0] + v[1] + alpha * e;
        }
    }
    Aff2 m = chunk_map2(tab, cnt, v[0], v[1]), tot;
    g.scan(m, tot);
    double x0, x1;
    m(ph, fr, x0, x1);                                               // state entering this thread's chunk
    bool bad = false;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        if (j < cnt) {
            const double e = c[j] - x0;
            const double f = x1 + beta * e;
            bad = bad || !(fabs(e) < 0.4999) || !(f >= lo && f <= hi);
            emit(base + j, x0, f);
            x1 = f;
            x0 = x0 + f + alpha * e;
        }
    }
#ifdef PC_CENSUS
    g.cen_or((g.any(bad) ? 1u << 18 : 0u) | (g.any(zero) ? 1u << 19 : 0u));
#endif
    if (g.any(bad || zero)) return false;
#ifdef PC_CENSUS
    g.cen_or(1u << 16);
#endif
    double nph, nfr;
    tot(ph, fr, nph, nfr);
    ph = nph - rint(nph); fr = nfr;
    return true;
}

// The same loop where that guess does not hold for a whole tile -- no carrier (an idle channel: the phase is noise),
// cycle slips, the frequency clamp at work.  Every thread walks the EXACT recurrence over its LC samples, started
// `warm` samples early from a zero state.  The loop is a contraction: a state error shrinks by its spectral radius
// rho every sample (CFmDemod at 62.5 kHz: 0.47), a wrap moves the phase by whole turns only and a clamped frequency
// is exact at once -- so by its first own sample a thread's state has met the sequential one.  That is checked, not
// assumed: a thread's start state must equal its predecessor's end state to 1e-9 turns (the first threads start
// from the true state at sample 0), and then by induction every state is the sequential one TO THAT BOUND -- not bit
// for bit: the audio of an accepted tile may differ from the one-thread walk's by rounding (tests: 1e-6 of full scale;
// include/cutesdr_mi.h states the contract).  Any mismatch -> false, and the caller walks the tile.  warm = pll_warm_len() samples: rho^(warm-8) < 1e-13; the eight
// on top are for a wrap decision that differs late in the warm-up (measured on noise: 32 samples at rho = 0.47 sent
// a quarter of the tiles to the one-thread walk, 48 none: 1.92 -> 0.45 ms for 85 idle receivers x 2^20 samples, against
// 0.34 ms with carriers).
// xp, xf: NT doubles of LDS each.  emit(i, phase_before, freq_after).  ph, fr are written only on success.
__device__ __forceinline__ int pll_warm_len(double alpha, double beta)
{
    const double tr = 2.0 - alpha - beta, det = 1.0 - alpha, disc = tr * tr - 4.0 * det;
    const double rho = disc < 0.0 ? sqrt(fabs(det)) : 0.5 * (fabs(tr) + sqrt(disc));
    if (!(rho > 0.0)) return 8;
    if (!(rho < 0.98)) return 1 << 20;
    return (int)(-30.0 / log(rho)) + 10;
}
template <int NW, class F>
__device__ __forceinline__ bool pll_overlap(const Wg<NW> &g, const float *th, int n, int warm, double alpha, double beta, double lo,
                                            double hi, double &ph, double &fr, double *xp, double *xf, F emit)
{
    constexpr int LC = Wg<NW>::LC;
    const int base = g.base(), cnt = g.count(n);
    int i = base - warm;
    double p = 0.0, f = 0.0;
    const bool exact = i <= 0;
    if (exact) { i = 0; p = ph; f = fr; }
    if (cnt > 0) {
        float v = th[i];
        for (; i < base; i++) { const float vn = th[i + 1]; pll_step(v, p, f, alpha, beta, lo, hi, 1.0); v = vn; }
    }
    const double ps = p, fs = f;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        if (j < cnt) { const double pb = p; pll_step(th[base + j], p, f, alpha, beta, lo, hi, 1.0); emit(base + j, pb, f); }
    }
    xp[g.t] = p; xf[g.t] = f;
    g.sync();
    bool bad = false;
    if (cnt > 0 && !exact) {
        const double dp = ps - xp[g.t - 1], df = fs - xf[g.t - 1];
        bad = !(fabs(dp - rint(dp)) < 1e-9) || !(fabs(df) < 1e-9);
    }
    const int tl = n > 0 ? (n - 1) / LC : 0;
    const double pe = xp[tl], fe = xf[tl];
#ifdef PC_CENSUS
    if (g.cen_fail_overlap) { g.cen_rec |= 1u << 23; bad = true; }
#endif
    if (g.any(bad)) return false;
#ifdef PC_CENSUS
    g.cen_or(2u << 16);
#endif
    if (n > 0) { ph = pe; fr = fe; }
    return true;
}

// The same loop where neither holds: thread 0 walks the tile sample by sample and every thread gets the end state.
// ph, fr, lo, hi in radians, as the channel keeps them; emit(i, phase_before, freq_after) in turns.
template <int NW, class F>
__device__ __forceinline__ void pll_walk(const Wg<NW> &g, const float *th, int n, double alpha, double beta, double lo, double hi,
                                         double sgn, double &ph, double &fr, F emit)
{
#ifdef PC_CENSUS
    g.cen_or(3u << 16);
#endif
    g.sync();
    if (g.t == 0) {
        const double lo_t = lo * kInvTwoPiD, hi_t = hi * kInvTwoPiD;
        double p = ph * kInvTwoPiD, f = fr * kInvTwoPiD;
        seq_walk(th, n, [&](float v, int i) {
            const double pb = p;
            pll_step(v, p, f, alpha, beta, lo_t, hi_t, sgn);
            emit(i, pb, f);
        });
        ph = p * kTwoPiD; fr = f * kTwoPiD;
    }
    ph = g.bcast0(ph, 0); fr = g.bcast0(fr, 1);
}

// pk[i] = max(E[i .. i+W1]), i < n, for E = S.mg[0 .. W1+n).  Chunks of 16: per-chunk prefix and
// suffix maxima (registers), a log table over the <= 192 chunk maxima for the chunks strictly
// inside a window, then window = suffix(first chunk) | inner chunks | prefix(last chunk).
// Only prefix values at tile positions (-> S.pk) and suffix values at i < n (-> S.w2) are kept.
template <int NW, class L>
__device__ __forceinline__ void sliding_max(const Wg<NW> &g, L &S, int W1, int n)
{
    constexpr int NT = Wg<NW>::NT;
    const int len = W1 + n, t = g.t;
    if (W1 < 16) {                                      // short windows: direct
        for (int i = t; i < n; i += NT) {
            float v = S.mg[i];
            for (int k = 1; k <= W1; k++) v = fmaxf(v, S.mg[i + k]);
            S.pk[i] = v;
        }
        g.sync();
        return;
    }
    const int nc = (len + 15) >> 4;
    for (int c = t; c < PC_NCHUNK; c += NT) {
        float e[16];
        const float4 *src = reinterpret_cast<const float4 *>(S.mg + 16 * c);
        if (c < nc) {
#pragma unroll
            for (int q = 0; q < 4; q++) { const float4 v = src[q]; e[4 * q] = v.x; e[4 * q + 1] = v.y; e[4 * q + 2] = v.z; e[4 * q + 3] = v.w; }
#pragma unroll
            for (int j = 0; j < 16; j++) if (16 * c + j >= len) e[j] = kNegBig;
            float pre[16], suf[16];
            pre[0] = e[0]; suf[15] = e[15];
#pragma unroll
            for (int j = 1; j < 16; j++) { pre[j] = fmaxf(pre[j - 1], e[j]); suf[15 - j] = fmaxf(suf[16 - j], e[15 - j]); }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const int idx = 16 * c + j;
                const int ip = idx - W1;                                  // prefix wanted at tile positions
                S.pk[(ip >= 0 && ip < n) ? ip : PT + 15] = pre[j];
                S.w2[idx < n ? idx : PT + 15] = suf[j];
            }
            S.rt[0][c] = pre[15];
        } else {
            S.rt[0][c] = kNegBig;
        }
    }
    g.sync();
    for (int l = 1; l < PC_RLEVELS; l++) {
        const int h = 1 << (l - 1);
        for (int c = t; c < PC_NCHUNK; c += NT) {
            const float v0 = S.rt[l - 1][c];
            const float v1 = (c + h < PC_NCHUNK) ? S.rt[l - 1][c + h] : kNegBig;
            S.rt[l][c] = fmaxf(v0, v1);
        }
        g.sync();
    }
    for (int i = t; i < n; i += NT) {
        const int ci = i >> 4, ce = (i + W1) >> 4, cnt = ce - ci - 1;     // W1 >= 16: ce > ci
        float v = fmaxf(S.w2[i], S.pk[i]);
        if (cnt > 0) {
            const int l = 31 - __clz(cnt);
            v = fmaxf(v, fmaxf(S.rt[l][ci + 1], S.rt[l][ce - (1 << l)]));
        }
        S.pk[i] = v;
    }
    g.sync();
}

#ifndef CSDR_PC_WAVES_PER_EU
#define CSDR_PC_WAVES_PER_EU 1
#endif
// LEAN: the walk of a chain call of several bursts, where everything without feedback has left it -- no S-meter
// (smeter_call_kernel), the AGC's peaks from agc_peaks_kernel (PC_AGC_PRE), FM's squelch half deferred (PC_FM_DEFER).
// The code those stages needed is compiled out: it never ran in such a launch, but its live ranges set the kernel's
// register allocation (256 + 118 for the full kernel: one workgroup per CU and nothing but one down-converter wave
// beside it on a SIMD).
#ifndef CSDR_PC_LEAN_WAVES_PER_EU
#define CSDR_PC_LEAN_WAVES_PER_EU 2
#endif

// What a thread of the walk knows about its launch and its channel: constant over the tile loop.
template <int NW, bool LEAN>
struct PcThread {
    static constexpr int NT = Wg<NW>::NT, LC = Wg<NW>::LC;
    static constexpr bool kPrefetch = NW > 1;   // with several waves per channel a tile's samples are fetched into registers
                                                // one tile ahead (a channel's workgroup usually has its CU to itself: nothing
                                                // else would hide the HBM latency)
    const PcArgs &a;
    PcLds &S;
    int t;
    Wg<NW> g;
    PcChannel &C;
    float *g_dly, *g_mag;               // linear: last dly_n inputs, oldest first; last win_n-1 magnitudes
    const float2 *in;
    bool stereo;
    PcRow row;
    int mode;
    bool do_sm, do_agc, agc_real, cpx_out;
    bool defer;                         // FM with the squelch deferred: this walk ends at the raw audio (fm_squelch_launch
                                        // does the rest, burst-parallel)
    bool pre;                           // AGC peaks from agc_peaks_kernel: the walk neither computes nor keeps the window's
                                        // log magnitudes
    const float *pkrow;                 // ... but reads the channel's peaks from here
    int D, W1, fm_warm;
    const PcFir *fir;                   // the active demodulator's FIR, if it has one
    int nt;
    long total;
};
template <int NW, bool LEAN>
__device__ __forceinline__ PcThread<NW, LEAN> pc_thread(const PcArgs &a, PcLds &S, int ch, int t)
{
    PcChannel &C = a.chan[ch];
    const bool stereo = a.flags & PC_STEREO;
    const PcRow row = a.out ? PcRow::of(a, ch) : PcRow{nullptr, nullptr, stereo};
    const int mode = (a.flags & PC_DO_DEMOD) ? C.mode : PC_MODE_NONE;
    const bool do_sm = !LEAN && (a.flags & PC_DO_SMETER), do_agc = a.flags & PC_DO_AGC, agc_real = !LEAN && (a.flags & PC_AGC_REAL);
    const bool defer = LEAN ? mode == PC_MODE_FM : ((a.flags & PC_FM_DEFER) && mode == PC_MODE_FM && a.burst <= 16384);
    const bool pre = LEAN ? (do_agc && C.agc.on) : ((a.flags & PC_AGC_PRE) && do_agc && C.agc.on && !agc_real);
    const float *pkrow = pre ? a.pkbuf + (long)ch * a.nbursts * a.burst : nullptr;
    const int D = C.agc.dly_n > 0 ? C.agc.dly_n : 1, W1 = C.agc.win_n > 0 ? C.agc.win_n - 1 : 0;
    const int fm_warm = mode == PC_MODE_FM ? pll_warm_len(C.fm.alpha, C.fm.beta) : 0;
    const PcFir *fir = mode == PC_MODE_AM ? &C.am.fir : mode == PC_MODE_SAM ? &C.sam.fir : mode == PC_MODE_FM ? &C.fm.hp : nullptr;
    return {a, S, t, {t, t & 63, t >> 6, &S.sy}, C,
            a.agc_dly + (long)ch * PC_AGC_RING * 2, a.agc_mag + (long)ch * PC_AGC_RING,
            reinterpret_cast<const float2 *>(a.in) + (long)ch * a.in_stride,
            stereo, row, mode, do_sm, do_agc, agc_real, stereo || mode == PC_MODE_NONE, defer, pre, pkrow,
            D, W1, fm_warm, fir, fir ? fir->ntaps : 1, (long)a.nbursts * a.burst};
}

#ifdef PC_PROFILE
#define PC_TICK(k) do { const unsigned long long now_ = __builtin_readcyclecounter(); st.tk[k] += now_ - st.tlast; st.tlast = now_; } while (0)
#else
#define PC_TICK(k)
#endif
// This thread's own registers: arrays, kept apart from the scalars of PcState so that those become values at once.
template <int NW>
struct PcRegs {
    float lp_y[Wg<NW>::LC];             // one-tile FM burst: its low-passed audio, kept until the squelch decision
    float2 nxt[Wg<NW>::LC];             // the prefetched tile
    float nxp[Wg<NW>::LC];              // PC_AGC_PRE: the tile's peaks travel with its samples
};
// The running state of the channel, identical on every thread, in the order the kernel fills it from PcChannel
struct PcState {
    PcSMeter sm;
    PcAgc agc;
    double am_z1;
    double sam_z1, sam_y1, sam_ph, sam_fr;
    double fm_ph, fm_fr, fm_dc, fm_sq;
    int fm_squelched;
    PcIir lp;
    double lp_w1, lp_w2;                // one-tile FM burst: the low-pass state behind it, kept until the squelch decision
#ifdef PC_PROFILE
    unsigned long long tk[16], tlast;   // (tk: zero from the kernel's initialiser)
#endif
};

// AGC rings, FIR taps and delay line, power / biquad / PLL tables -> LDS
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_stage_histories(const PcThread<NW, LEAN> &c, const PcState &st)
{
    constexpr int NT = Wg<NW>::NT;
    PcLds &S = c.S; const PcChannel &C = c.C; const PcFir *fir = c.fir;
    const int t = c.t, mode = c.mode, nt = c.nt;
    if (c.do_agc && st.agc.on) {
        for (int i = t; i < c.D; i += NT) S.dl[i] = make_float2(c.g_dly[2 * i], c.g_dly[2 * i + 1]);
        if constexpr (!LEAN) if (!c.pre) for (int i = t; i < c.W1; i += NT) S.mg[i] = c.g_mag[i];
    }
    if (fir) {
        stage_taps<NT>(S.h0, (mode == PC_MODE_FM || !c.stereo) ? fir->coef : fir->icoef, nt, t);
        stage_taps<NT>(S.h1, fir->qcoef, nt, t);
        // behind the tile the FIR window reads up to three more samples: zeros, never written again
        for (int i = t; i < PT + PC_FIR_MAX + 17; i += NT) { S.w0[i] = 0.f; S.w1[i] = 0.f; }
        c.g.sync();
        for (int i = t; i < nt - 1; i += NT) { S.w0[i] = (mode == PC_MODE_FM || (mode == PC_MODE_AM && !c.stereo)) ? fir->zreal[i] : fir->zr[i]; S.w1[i] = fir->zi[i]; }
    }
    pow_table(S.pw_sm, 1.0 - st.sm.att_a, t);
    static_assert(refc::AM_DC_ALPHA == refc::SAM_DC_ALPHA, "one table of DC-blocker powers serves AM and SAM");
    pow_table(S.pw_dc, refc::AM_DC_ALPHA, t);
    pow_table(S.pw_sq, 1.0 - C.fm.sq_alpha, t);
    pow_table(S.pw_fd, 1.0 - C.fm.dc_alpha, t);
    biquad_table(S.bq, st.lp, t);
    if (mode == PC_MODE_FM) pll_table(S.pm, C.fm.alpha, C.fm.beta, t);
    if (mode == PC_MODE_SAM) pll_table(S.pm, C.sam.alpha, C.sam.beta, t);
    c.g.sync();
}

// cnt samples (and their peaks) from position g0 of the channel's input into this thread's registers
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_fetch(const PcThread<NW, LEAN> &c, PcRegs<NW> &r, long g0, int cnt)
{
    constexpr int NT = Wg<NW>::NT, LC = Wg<NW>::LC;
#pragma unroll
    for (int j = 0; j < LC; j++) { const int i = c.t + NT * j; if (i < cnt) { r.nxt[j] = c.in[g0 + i]; if (c.pre) r.nxp[j] = c.pkrow[g0 + i]; } }
}
// the tile at sample t0 of its burst (gi of the call) -> x[0..n), and the next one into the registers
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_load_tile(const PcThread<NW, LEAN> &c, PcRegs<NW> &r, float2 *x, int n, long gi, int t0)
{
    constexpr int NT = Wg<NW>::NT, LC = Wg<NW>::LC;
    const PcArgs &a = c.a; const int t = c.t;
    if (c.kPrefetch) {
#pragma unroll
        for (int j = 0; j < LC; j++) { const int i = t + NT * j; if (i < n) { x[i] = r.nxt[j]; if (c.pre) c.S.pk[i] = r.nxp[j]; } }
        const long gn = gi + n;                                // bursts are contiguous: the next tile follows
        if (gn < c.total) {
            const int left = a.burst - ((t0 + n) % a.burst);
            pc_fetch(c, r, gn, left < PT ? left : PT);
        }
    } else {
        for (int i = t; i < n; i += NT) x[i] = c.in[gi + i];
    }
    c.g.sync();
}

// S-meter (smeter.cpp:62-93)
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_smeter_stage(const PcThread<NW, LEAN> &c, PcState &st, const float2 *x, int n)
{
    constexpr int NT = Wg<NW>::NT; PcLds &S = c.S;
    if constexpr (!LEAN) if (c.do_sm) {
        for (int i = c.t; i < n; i += NT) {
            const float pw = (x[i].x * x[i].x + x[i].y * x[i].y) * refc::SM_INV_MAX_PWR_F;
            S.w2[i] = pw > 0.f ? 10.0f * log10f(pw) : -500.0f;
        }
        c.g.sync();
        smeter_tile(c.g, st.sm, S.w2, n, S.pw_sm);
        c.g.sync();
    }
}

// AGC (agc.cpp:174-296 / 301-401): x[0..n) in, the AGC output in place
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_agc_stage(const PcThread<NW, LEAN> &c, PcState &st, float2 *x, int n, long gi)
{
    constexpr int NT = Wg<NW>::NT, LC = Wg<NW>::LC;
    PcLds &S = c.S; PcAgc &agc = st.agc; const Wg<NW> &g = c.g; const int t = c.t;
    if (!c.do_agc) return;
#ifdef PC_CENSUS
    if (!agc.on) g.cen_or(1u);
#endif
    if (!agc.on) {
        const float gm = (float)agc.manual_gain;
        for (int i = t; i < n; i += NT) { x[i].x *= gm; x[i].y *= gm; }
        g.sync();
    } else {
        if (c.pre) {
            if (!c.kPrefetch) { for (int i = t; i < n; i += NT) S.pk[i] = c.pkrow[gi + i]; g.sync(); }
        } else if constexpr (!LEAN) {
            float *mg = S.mg + c.W1;
            for (int i = t; i < n; i += NT) {
                float m = fabsf(x[i].x);
                if (!c.agc_real) { const float mi = fabsf(x[i].y); if (mi > m) m = mi; }
                mg[i] = log10f(m + refc::AGC_MIN_CONSTANT_F) - refc::AGC_LOG10_MAX_AMPLITUDE_F;
            }
            g.sync();
            // sliding maximum: pk[i] = max E[i .. i+W1], E = [W1 history | tile] = S.mg
            PC_TICK(2);
            sliding_max(g, S, c.W1, n);
            PC_TICK(3);
            keep_tail(g, S.mg, c.W1, n);                      // the last W1 magnitudes are the next tile's history
            g.sync();
        }
        PC_TICK(4);
        // attack / decay averagers -> log gain argument max(att, dec) per sample in S.pk
        {
            double att = agc.attack_ave, dec = agc.decay_ave;
            bool ok = !agc.hang;                              // the hang timer is a counter: walked
            if constexpr (NW == 4) {           // (16 samples per thread would not fit the registers twice)
                if (ok) ok = agc_ave_scan2(g, S.pk, n, agc.att_rise, agc.att_fall, agc.dec_rise, agc.dec_fall, att, dec,
                                           [&](int i, double va, double vd) { S.pk[i] = fmaxf((float)va, (float)vd); });
#ifdef PC_CENSUS
                if (ok) g.cen_or(2u | (unsigned)g.cen_rounds << 4);
#endif
            } else {
                if (ok) ok = agc_ave_scan(g, S.pk, n, agc.att_rise, agc.att_fall, att,
                                          [&](int i, double v) { S.w2[i] = (float)v; });
#ifdef PC_CENSUS
                const bool cen_first = ok;
                if (!agc.hang) g.cen_or(ok ? (unsigned)g.cen_rounds << 4 : 1u << 12);
#endif
                if (ok) ok = agc_ave_scan(g, S.pk, n, agc.dec_rise, agc.dec_fall, dec,
                                          [&](int i, double v) { S.pk[i] = fmaxf(S.w2[i], (float)v); });
#ifdef PC_CENSUS
                if (cen_first) g.cen_or(ok ? (2u | (unsigned)g.cen_rounds << 8) : 2u << 12);
#endif
            }
#ifdef PC_CENSUS
            if (!ok) g.cen_or(agc.hang ? 3u : 4u);
#endif
            if (ok) { agc.attack_ave = att; agc.decay_ave = dec; }
            else {
                g.sync();
                att = agc.attack_ave; dec = agc.decay_ave;
                int timer = agc.hang_timer;
                if (t == 0) {
                    const double ar = agc.att_rise, af = agc.att_fall, dr = agc.dec_rise, df = agc.dec_fall;
                    const bool hang = agc.hang;
                    const int hang_time = agc.hang_time;
                    float *dst = S.pk;
                    seq_walk(S.pk, n, [&](float v, int i) {
                        const double pk = v;
                        const double da = pk - att, dd = pk - dec;
                        att = att + (da > 0.0 ? ar : af) * da;
                        const bool up = dd > 0.0, hold = hang && !up && timer < hang_time;
                        dec = dec + (up ? dr : (hold ? 0.0 : df)) * dd;
                        if (hang) timer = up ? 0 : (hold ? timer + 1 : timer);
                        dst[i] = (float)fmax(att, dec);
                    });
                }
                agc.attack_ave = g.bcast0(att, 0); agc.decay_ave = g.bcast0(dec, 1);
                agc.hang_timer = (int)g.bcast0((double)timer, 2);
            }
        }
        g.sync();
        PC_TICK(5);
        // gain law + delay line: out[i] = in[i - D] * gain[i]; S.dl = [D old | n new]
        const float knee = (float)agc.knee, slm1 = (float)(agc.gain_slope - 1.0), fixed_gain = (float)agc.fixed_gain;
        float2 outv[LC];
#pragma unroll
        for (int j = 0; j < LC; j++) {
            const int i = t + NT * j;
            if (i < n) {
                const float m = S.pk[i];
                const float gv = (m <= knee) ? fixed_gain : 0.7f * exp10f(m * slm1);
                const float2 d = S.dl[i];
                outv[j] = make_float2(d.x * gv, d.y * gv);
            }
        }
        keep_tail(g, S.dl, c.D, n);
#pragma unroll
        for (int j = 0; j < LC; j++) { const int i = t + NT * j; if (i < n) x[i] = outv[j]; }
        g.sync();
    }
}

// no demodulator, or SSB / CW: the AGC output is the audio (ssbdemod.cpp:48-53)
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_ssb_tile(const PcThread<NW, LEAN> &c, const float2 *x, int n, long gi)
{
    if (c.a.out)
        for (int i = c.t; i < n; i += Wg<NW>::NT) { if (c.cpx_out) c.row.s[gi + i] = x[i]; else c.row.m[gi + i] = x[i].x; }
    c.g.sync();
}

// CAmDemod (amdemod.cpp:66-104)
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_am_tile(const PcThread<NW, LEAN> &c, PcState &st, const float2 *x, int n, long gi)
{
    constexpr int NT = Wg<NW>::NT, LC = Wg<NW>::LC;
    PcLds &S = c.S; const Wg<NW> &g = c.g; const int t = c.t, nt = c.nt;
    float *w = S.w0 + (nt - 1);
    for (int i = t; i < n; i += NT) w[i] = sqrtf(x[i].x * x[i].x + x[i].y * x[i].y);
    g.sync();
    // DC block z0 = x + 0.99 z1, out = z0 - z1 (amdemod.cpp:70-80)
    st.am_z1 = lin1_scan<true>(g, w, n, refc::AM_DC_ALPHA, 1.0, st.am_z1, S.pw_dc,
                               [&](int i, float, double z0, double z1) { w[i] = (float)(z0 - z1); });
    g.sync();
    float acc[LC], acq[LC];
    fir_blk<NW>(S.h0, nt, S.w0, t, acc);
    if (c.stereo) {
        fir_blk<NW>(S.h1, nt, S.w0, t, acq);
#pragma unroll
        for (int j = 0; j < LC; j++) { const int i = pc_out_index<NW>(t, j); if (i < n) c.row.s[gi + i] = make_float2(acc[j], acq[j]); }
    } else {
#pragma unroll
        for (int j = 0; j < LC; j++) { const int i = pc_out_index<NW>(t, j); if (i < n) c.row.m[gi + i] = acc[j]; }
    }
    g.sync();
    slide(g, S.w0, nt - 1, n);
    g.sync();
}

// CFmDemod (fmdemod.cpp:113-236) up to the end-of-burst squelch
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_fm_tile(const PcThread<NW, LEAN> &c, PcState &st, PcRegs<NW> &r, const float2 *x, int n, long gi)
{
    constexpr int NT = Wg<NW>::NT, LC = Wg<NW>::LC;
    PcLds &S = c.S; const PcArgs &a = c.a; const Wg<NW> &g = c.g; const int t = c.t, nt = c.nt;
    float *th = S.w1 + (nt - 1), *au = S.w0 + (nt - 1);
    const PcFm &F = c.C.fm;
    const auto to_au = [&](int i, double, double f) { au[i] = (float)f; };           // NCO frequency, turns per sample
    double ph = st.fm_ph * kInvTwoPiD, fr = st.fm_fr * kInvTwoPiD;                   // (the solvers move them only when they succeed)
    bool scanned = pll_scan(g, th, n, F.alpha, F.beta, F.lo * kInvTwoPiD, F.hi * kInvTwoPiD, ph, fr, S.pm, to_au);
#ifdef PC_CENSUS
    if (!scanned) g.cen_or((c.fm_warm > PC_PLL_WARM_MAX ? 1u << 21 : 0u) | ((a.flags & PC_PLL_SEQ) ? 1u << 22 : 0u));
#endif
    if (!scanned && c.fm_warm <= PC_PLL_WARM_MAX && !(a.flags & PC_PLL_SEQ)) {       // unlocked: overlapped exact walks, verified
        g.sync();
        ph = wrap_turn(ph);
        scanned = pll_overlap(g, th, n, c.fm_warm, F.alpha, F.beta, F.lo * kInvTwoPiD, F.hi * kInvTwoPiD, ph, fr,
                              reinterpret_cast<double *>(&S.rt[0][0]), reinterpret_cast<double *>(S.w2), to_au);
    }
    if (scanned) { st.fm_ph = ph * kTwoPiD; st.fm_fr = fr * kTwoPiD; }
    else pll_walk(g, th, n, F.alpha, F.beta, F.lo, F.hi, 1.0, st.fm_ph, st.fm_fr, to_au);
    g.sync();
    PC_TICK(8);
    {   // audio = (freq - its running mean) * gain  (fmdemod.cpp:178-186): the mean is linear
        const double og = F.out_gain * kTwoPiD;
        st.fm_dc = kTwoPiD * lin1_scan<true>(g, au, n, 1.0 - F.dc_alpha, F.dc_alpha, st.fm_dc * kInvTwoPiD, S.pw_fd,
                    [&](int i, float f, double dc, double) { au[i] = (float)(((double)f - dc) * og); });
    }
    g.sync();
    PC_TICK(9);
    // raw audio to the output row; squelch is decided at the end of the burst (a burst of one tile
    // keeps it in LDS instead: the low-pass at the end of the burst reads it from there)
    if (a.burst > PT || c.defer)
        for (int i = t; i < n; i += NT) c.row.put(gi + i, au[i]);
    if constexpr (!LEAN) if (a.burst <= 16384 && !c.defer) {                     // MAX_SQBUF_SIZE
        float acc[LC];
        fir_blk<NW>(S.h0, nt, S.w0, t, acc);
#pragma unroll
        for (int j = 0; j < LC; j++) S.w2[pc_out_index<NW>(t, j) & (PT - 1)] = fabsf(acc[j]);
        g.sync();
        if constexpr (NW == 4) {
            if (a.burst <= PT) st.fm_sq = sq_and_lowpass(g, S.w2, au, n, 1.0 - F.sq_alpha, F.sq_alpha, st.fm_sq, S.pw_sq, st.lp, S.bq,
                                                         r.lp_y, st.lp_w1, st.lp_w2);
            else st.fm_sq = lin1_scan<false>(g, S.w2, n, 1.0 - F.sq_alpha, F.sq_alpha, st.fm_sq, S.pw_sq,
                                             [](int, float, double, double) {});
        } else
        st.fm_sq = lin1_scan<false>(g, S.w2, n, 1.0 - F.sq_alpha, F.sq_alpha, st.fm_sq, S.pw_sq,
                                    [](int, float, double, double) {});
    }
    g.sync();
    PC_TICK(10);
    if (!c.defer) {
        slide(g, S.w0, nt - 1, n);
        g.sync();
    }
    PC_TICK(11);
}

// CSamDemod (samdemod.cpp:78-158)
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_sam_tile(const PcThread<NW, LEAN> &c, PcState &st, const float2 *x, int n, long gi)
{
    constexpr int NT = Wg<NW>::NT, LC = Wg<NW>::LC;
    PcLds &S = c.S; const Wg<NW> &g = c.g; const int t = c.t, nt = c.nt; const bool stereo = c.stereo;
    float *th = S.w1 + (nt - 1), *au = S.w0 + (nt - 1);
    const PcSam &M = c.C.sam;
    const double sgn = stereo ? 1.0 : -1.0;
    // in psi = sgn phi, g = sgn f the loop has the FM form with theta as is
    double ps = sgn * st.sam_ph * kInvTwoPiD, gf = sgn * st.sam_fr * kInvTwoPiD;
    const double l0 = M.lo * kInvTwoPiD, h0 = M.hi * kInvTwoPiD;
    if (pll_scan(g, th, n, M.alpha, M.beta, sgn > 0 ? l0 : -h0, sgn > 0 ? h0 : -l0, ps, gf, S.pm,
                 [&](int i, double p, double) { S.w2[i] = (float)(sgn * (p - rint(p))); })) {
        st.sam_ph = sgn * ps * kTwoPiD; st.sam_fr = sgn * gf * kTwoPiD;
    } else pll_walk(g, th, n, M.alpha, M.beta, M.lo, M.hi, sgn, st.sam_ph, st.sam_fr,
                           [&](int i, double p, double) { S.w2[i] = (float)p; });     // phase used for this sample (turns)
    g.sync();
    // rotated sample tr + j ti = |x| e^{j(theta + sgn phi)}
    for (int i = t; i < n; i += NT) {
        const float r = sqrtf(x[i].x * x[i].x + x[i].y * x[i].y);
        float sn, cs;
        sincospif(2.0f * (th[i] + (float)sgn * S.w2[i]), &sn, &cs);
        au[i] = r * cs;                                   // tr
        th[i] = r * sn;                                   // ti
    }
    g.sync();
    // DC blocks
    st.sam_z1 = lin1_scan<true>(g, au, n, refc::SAM_DC_ALPHA, 1.0, st.sam_z1, S.pw_dc,
                                [&](int i, float, double z0, double z1) { au[i] = (float)(z0 - z1); });
    if (stereo)
        st.sam_y1 = lin1_scan<true>(g, th, n, refc::SAM_DC_ALPHA, 1.0, st.sam_y1, S.pw_dc,
                                    [&](int i, float, double y0, double y1) { th[i] = (float)(y0 - y1); });
    g.sync();
    if (!stereo) {
        for (int i = t; i < n; i += NT) c.row.m[gi + i] = au[i];
    } else {
        float ar[LC], ai[LC];
        fir_blk<NW>(S.h0, nt, S.w0, t, ar);
        fir_blk<NW>(S.h1, nt, S.w1, t, ai);
#pragma unroll
        for (int j = 0; j < LC; j++) {                    // lower sideband left, upper right
            const int i = pc_out_index<NW>(t, j);
            if (i < n) c.row.s[gi + i] = make_float2(ar[j] + ai[j], ar[j] - ai[j]);
        }
        g.sync();
        slide(g, S.w0, nt - 1, n);
        slide(g, S.w1, nt - 1, n);
    }
    g.sync();
}

// end of burst b: FM squelch decision (fmdemod.cpp:128-151), then zeros or the audio low-pass over the burst
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_fm_burst_end(const PcThread<NW, LEAN> &c, PcState &st, const PcRegs<NW> &r, int b)
{
    constexpr int NT = Wg<NW>::NT, LC = Wg<NW>::LC;
    PcLds &S = c.S; const PcArgs &a = c.a; const Wg<NW> &g = c.g; const int t = c.t;
    if constexpr (!LEAN) if (c.mode == PC_MODE_FM && a.burst <= 16384 && !c.defer) {
        st.fm_squelched = squelch_decide(st.fm_sq, c.C.fm.sq_thresh, st.fm_squelched);
        const long g0 = (long)b * a.burst;
        g.sync();
        for (int t0 = 0; t0 < a.burst; t0 += PT) {
            const int n = (a.burst - t0) < PT ? (a.burst - t0) : PT;
            if (st.fm_squelched) {
                for (int i = t; i < n; i += NT) c.row.put(g0 + t0 + i, 0.f);
            } else if (NW == 4 && a.burst <= PT) {                    // the low-pass ran with the squelch average: commit it
#pragma unroll
                for (int j = 0; j < LC; j++) {
                    const int i = LC * t + j;
                    if (i < n) c.row.put(g0 + i, r.lp_y[j]);
                }
                st.lp.w1a = st.lp_w1; st.lp.w2a = st.lp_w2;
            } else {                                                  // low-pass biquad over the burst
                if (a.burst > PT) { for (int i = t; i < n; i += NT) S.w2[i] = c.row.raw(g0 + t0 + i); }
                else { const float *au = S.w0 + (c.nt - 1); for (int i = t; i < n; i += NT) S.w2[i] = au[i]; }
                g.sync();
                biquad_scan(g, S.w2, n, st.lp, S.bq);
                g.sync();
                for (int i = t; i < n; i += NT) c.row.put(g0 + t0 + i, S.w2[i]);
                g.sync();
            }
        }
    }
}

// write the state back
template <int NW, bool LEAN>
__device__ __forceinline__ void pc_store_state(const PcThread<NW, LEAN> &c, const PcState &st, int ch)
{
    constexpr int NT = Wg<NW>::NT;
    PcLds &S = c.S; PcChannel &C = c.C; const int t = c.t, mode = c.mode;
    c.g.sync();
    if (c.do_agc && st.agc.on) {
        for (int i = t; i < c.D; i += NT) { c.g_dly[2 * i] = S.dl[i].x; c.g_dly[2 * i + 1] = S.dl[i].y; }
        if (c.pre) { const float *tail = c.a.magtail + (long)ch * PC_AGC_RING; for (int i = t; i < c.W1; i += NT) c.g_mag[i] = tail[i]; }
        else if constexpr (!LEAN) for (int i = t; i < c.W1; i += NT) c.g_mag[i] = S.mg[i];
    }
    if (c.fir && !c.defer) {
        PcFir *fw = const_cast<PcFir *>(c.fir);
        for (int i = t; i < c.nt - 1; i += NT) {
            if (mode == PC_MODE_FM || (mode == PC_MODE_AM && !c.stereo)) fw->zreal[i] = S.w0[i];
            else { fw->zr[i] = S.w0[i]; fw->zi[i] = mode == PC_MODE_AM ? S.w0[i] : S.w1[i]; }
        }
    }
    // each stage writes only its own state: the stages of one channel may run as separate,
    // concurrent launches (S-meter | AGC | demodulator pipeline of the batch chain)
    if (t == 0) {
        if (c.do_sm) C.sm = st.sm;
        if (c.do_agc) C.agc = st.agc;
        if (mode == PC_MODE_AM) C.am.z1 = st.am_z1;
        if (mode == PC_MODE_SAM) { C.sam.z1 = st.sam_z1; C.sam.y1 = st.sam_y1; C.sam.phase = st.sam_ph; C.sam.freq = st.sam_fr; }
        if (mode == PC_MODE_FM) {
            C.fm.phase = st.fm_ph; C.fm.freq = st.fm_fr; C.fm.err_dc = st.fm_dc;
            if (!c.defer) { C.fm.sq_ave = st.fm_sq; C.fm.squelched = st.fm_squelched; C.fm.lp = st.lp; }   // else: fm_squelch_decide_kernel's
        }
    }
}

template <int NW, bool LEAN>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(NW == 4 ? (LEAN ? CSDR_PC_LEAN_WAVES_PER_EU : CSDR_PC_WAVES_PER_EU) : 1)))
void postchain_kernel(PcArgs a)
{
    CSDR_WG_TRACE_SCOPE(a.trace, WGT_WALK);
    extern __shared__ __attribute__((aligned(16))) unsigned char pc_smem[];
    PcLds &S = *reinterpret_cast<PcLds *>(pc_smem);
    const int ch = blockIdx.x;
#ifdef PC_CENSUS
    unsigned *const cen = a.census.buf;
    if (cen && ch == 0 && threadIdx.x == 0) { cen[3] = (unsigned)a.census.inst; cen[4] = (unsigned)(a.census.base + a.channels * a.census.tiles); cen[5] = (unsigned)a.census.launch; }
#endif
    // A channel's bursts are a sequential walk: this kernel is bound by its own latency, not by throughput, and
    // in the batch chain it shares CUs with the down-converter of other groups / the next call, whose 12-16 waves
    // per CU would otherwise take most issue slots.  Highest issue priority for these few waves costs the
    // streaming kernel next to nothing and keeps the walk at the speed it has alone.
    if (a.out_rows && a.out_rows[ch] < 0) return;      // muted row (its receiver has moved on): uniform per workgroup
    __builtin_amdgcn_s_setprio(3);
    const PcThread<NW, LEAN> c = pc_thread<NW, LEAN>(a, S, ch, threadIdx.x);
    const PcChannel &C = c.C;
    PcState st{C.sm, C.agc, C.am.z1, C.sam.z1, C.sam.y1, C.sam.phase, C.sam.freq, C.fm.phase, C.fm.freq, C.fm.err_dc, C.fm.sq_ave,
               C.fm.squelched, C.fm.lp, 0.0, 0.0};
    PcRegs<NW> r;
#ifdef PC_CENSUS
    const unsigned cen_force = cen ? (unsigned)__builtin_amdgcn_readfirstlane((int)cen[2]) : 0u;
    c.g.cen_force = cen_force;
    c.g.cen_limit = (cen_force & 15u) ? (int)(cen_force & 15u) - 1 : PC_AGC_ROUNDS;
    int cen_tile = 0;
#endif
    pc_stage_histories(c, st);
    if (c.kPrefetch && c.total > 0) pc_fetch(c, r, 0, a.burst < PT ? a.burst : PT);
#ifdef PC_PROFILE
    st.tlast = __builtin_readcyclecounter();
#endif
#pragma unroll
    for (int j = 0; j < c.LC; j++) r.lp_y[j] = 0.f;
    for (int b = 0; b < a.nbursts; b++) {
        for (int t0 = 0; t0 < a.burst; t0 += PT) {
            const int n = (a.burst - t0) < PT ? (a.burst - t0) : PT;
            const long gi = (long)b * a.burst + t0;
            float2 *x = S.dl + ((c.do_agc && st.agc.on) ? c.D : 0);       // tile samples (AGC: behind the delay history)
#ifdef PC_CENSUS
            c.g.cen_rec = 0;
            { const unsigned fm = cen_force >> 8 & 255u, fr = cen_force >> 16 & 255u;
              c.g.cen_fail_overlap = fm != 0 && (unsigned)(a.census.tile0 + cen_tile) % fm == fr; }
#endif
            pc_load_tile(c, r, x, n, gi, t0);
            PC_TICK(0);
            pc_smeter_stage(c, st, x, n);
            PC_TICK(1);
            pc_agc_stage(c, st, x, n, gi);
            PC_TICK(6);
            // x[0..n) now holds the AGC output (or the input)
            if (c.mode == PC_MODE_NONE || c.mode >= PC_MODE_USB) pc_ssb_tile(c, x, n, gi);
            else if (c.mode == PC_MODE_AM) pc_am_tile(c, st, x, n, gi);
            else {                                                        // PLL modes: theta = arg(x) for the whole tile, in turns
                float *th = S.w1 + (c.nt - 1);
                for (int i = c.t; i < n; i += c.NT) th[i] = pll_theta_of(x[i].x, x[i].y);
                c.g.sync();
                PC_TICK(7);
                if (c.mode == PC_MODE_FM) pc_fm_tile(c, st, r, x, n, gi);
                else pc_sam_tile(c, st, x, n, gi);
            }
#ifdef PC_CENSUS
            if (cen && c.t == 0) {                                        // this tile's record: one 16-byte vector store
                const int idx = a.census.base + ch * a.census.tiles + cen_tile;
                const int orow = a.out_rows ? a.out_rows[ch] : ch;
                if (idx >= 0 && (unsigned)idx < cen[1])
                    reinterpret_cast<uint4 *>(cen + 8)[idx] = make_uint4(c.g.cen_rec, (unsigned)n | (unsigned)(c.mode + 1) << 16 | (unsigned)a.census.inst << 20,
                        (unsigned)(a.census.launch & 0xffff) | (unsigned)(ch & 255) << 16 | (unsigned)(orow & 255) << 24,
                        (unsigned)(a.census.tile0 + cen_tile));
            }
            cen_tile++;
#endif
        }
        pc_fm_burst_end(c, st, r, b);
    }
    PC_TICK(12);
#ifdef PC_PROFILE
    if (blockIdx.x == 0 && c.t == 0)
        printf("pcprof mode %d: load %llu smeter %llu agcmag %llu slmax %llu histmove %llu aver %llu gain %llu atan %llu pll %llu dc %llu sqfir %llu slide %llu burstend %llu\n",
               c.mode, st.tk[0], st.tk[1], st.tk[2], st.tk[3], st.tk[4], st.tk[5], st.tk[6], st.tk[7], st.tk[8], st.tk[9], st.tk[10], st.tk[11], st.tk[12]);
#endif
    pc_store_state(c, st, ch);
}

// =====================================================================================================
// CAgc's log magnitudes and their sliding maximum (agc.cpp:196-231) for every sample of a call, ahead of the walk
// (PC_AGC_PRE).  Neither needs state from the loop -- only the win_n-1 magnitudes in front of a burst, which are
// the input's own -- so they leave the sequential walk (a fifth of an FM tile, a third of an SSB one) for one
// workgroup per (channel, group of bursts).  The same fp32 operations in the same order: the peaks, and with them
// every audio word, are what the walk computes itself.
// =====================================================================================================
__global__ __launch_bounds__(256)
void agc_peaks_kernel(PcArgs a)
{
    CSDR_WG_TRACE_SCOPE(a.trace, WGT_PEAKS);
    using G = Wg<4>;
    constexpr int NT = G::NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char pc_smem[];
    PreLds &S = *reinterpret_cast<PreLds *>(pc_smem);
    const PcBurstGroup bg = pc_burst_group(a.nbursts, a.pre_bpw);
    const int t = threadIdx.x, ch = bg.ch, b0 = bg.b0, b1 = bg.b1;
    if (a.out_rows && a.out_rows[ch] < 0) return;
    const PcChannel &C = a.chan[ch];
    if (!C.agc.on) return;                               // uniform per workgroup
    const G g{t, t & 63, t >> 6, &S.sy};
    const int W1 = C.agc.win_n > 0 ? C.agc.win_n - 1 : 0;
    const float2 *in = reinterpret_cast<const float2 *>(a.in) + (long)ch * a.in_stride;
    const float *g_mag = a.agc_mag + (long)ch * PC_AGC_RING;   // the last W1 magnitudes of the previous call
    float *pkrow = a.pkbuf + (long)ch * a.nbursts * a.burst;
    auto logmag = [](float2 v) {
        float m = fabsf(v.x);
        const float mi = fabsf(v.y);
        if (mi > m) m = mi;
        return log10f(m + refc::AGC_MIN_CONSTANT_F) - refc::AGC_LOG10_MAX_AMPLITUDE_F;     // agc.cpp:196-201
    };
    const long p0 = (long)b0 * a.burst, p1 = (long)b1 * a.burst, total = (long)a.nbursts * a.burst;
    // the window in front of this group's first sample
    for (int i = t; i < W1; i += NT) {
        const long k = p0 - W1 + i;
        S.mg[i] = k >= 0 ? logmag(in[k]) : g_mag[W1 + (int)k];
    }
    for (long pos = p0; pos < p1; ) {
        const long bend = (pos / a.burst + 1) * a.burst;  // tiles do not straddle bursts (as in the walk)
        const int n = (int)((bend - pos) < PT ? (bend - pos) : PT);
        float *mg = S.mg + W1;
        for (int i = t; i < n; i += NT) mg[i] = logmag(in[pos + i]);
        g.sync();
        sliding_max(g, S, W1, n);
        for (int i = t; i < n; i += NT) pkrow[pos + i] = S.pk[i];
        keep_tail(g, S.mg, W1, n);                       // the last W1 magnitudes are the next tile's window
        g.sync();
        pos += n;
    }
    if (p1 == total) {                                   // the window the next call starts with
        float *tail = a.magtail + (long)ch * PC_AGC_RING;
        for (int i = t; i < W1; i += NT) tail[i] = S.mg[i];
    }
}

hipError_t agc_peaks_launch(const PcArgs &a, hipStream_t stream)
{
#ifdef PC_CENSUS
    if (a.layout_tag != PC_ARGS_TAG) return hipErrorInvalidValue;   // the caller's unit was compiled without the macro
#endif
    static_assert(sizeof(PreLds) <= 40 * 1024, "four peaks workgroups per CU");
    PcArgs b = a;
    b.pre_bpw = pc_bursts_per_wg(a);
    const int ngrp = pc_burst_groups(a.nbursts, b.pre_bpw);
    hipLaunchKernelGGL(agc_peaks_kernel, dim3(a.channels * ngrp), dim3(256), sizeof(PreLds), stream, pc_traced(b));
    return hipGetLastError();
}

// =====================================================================================================
// CSMeter (smeter.cpp:62-93) over a WHOLE call, out of the walk (round 4).  The meter feeds nothing -- its averages
// go to the GUI -- and both of them are compositions of associative maps (the attack average an affine one, the decay
// average x -> max(A x + B, C)), so nothing about them is sequential: one workgroup per receiver takes the call in
// super-tiles of 8192 samples, a thread owning 32 CONSECUTIVE samples of a super-tile (power -> dB once, staged in
// LDS with a pad word every 32 so that both the coalesced fill and the per-thread runs are conflict-free), and pays
// two workgroup scans per 8192 samples where the walk paid two per 1024 -- a quarter to a half of a walked tile's
// time (S-meter alone as a walk: 4.5 us per 1024 samples, 290 us per call; here ~20 us).  The same fp64 maps as
// smeter_tile, chunked differently: states agree to rounding (1e-15 relative).
// =====================================================================================================
constexpr int SM_ST = 8192, SM_LC = SM_ST / 256;
struct SmLds {
    PcSync sy;
    alignas(16) float db[SM_ST + SM_ST / 32];
    double pw[SM_LC + 1];                                // (1 - att_a)^k
};
__global__ __launch_bounds__(256)
void smeter_call_kernel(PcArgs a)
{
    CSDR_WG_TRACE_SCOPE(a.trace, WGT_SMETER);
    using G = Wg<4>;
    __shared__ SmLds S;
    const int t = threadIdx.x, ch = blockIdx.x;
    if (a.out_rows && a.out_rows[ch] < 0) return;
    const G g{t, t & 63, t >> 6, &S.sy};
    PcChannel &C = a.chan[ch];
    PcSMeter sm = C.sm;
    const double aa = sm.att_a, ia = 1.0 - sm.att_a, da = sm.dec_a, id = 1.0 - sm.dec_a;
    if (t <= SM_LC) { double p = 1.0; for (int k = 0; k < t; k++) p *= ia; S.pw[t] = p; }
    const float2 *in = reinterpret_cast<const float2 *>(a.in) + (long)ch * a.in_stride;
    const long total = (long)a.nbursts * a.burst;
    for (long p0 = 0; p0 < total; p0 += SM_ST) {
        const int n = (int)((total - p0) < SM_ST ? (total - p0) : SM_ST);
        g.sync();                                        // the previous super-tile's runs have been read (and S.pw written)
        for (int i = t; i < n; i += 256) {
            const float2 v = in[p0 + i];
            const float pw = (v.x * v.x + v.y * v.y) * refc::SM_INV_MAX_PWR_F;
            S.db[i + (i >> 5)] = pw > 0.f ? 10.0f * log10f(pw) : -500.0f;
        }
        g.sync();
        const int base = SM_LC * t;
        int cnt = n - base; cnt = cnt < 0 ? 0 : (cnt > SM_LC ? SM_LC : cnt);
        const float *run = S.db + base + t;              // = index(base + j) for j < 32
        double p = 0.0, pk = -1.0e300;
        for (int j = 0; j < cnt; j++) { const double x = (double)run[j]; p = ia * p + aa * x; pk = fmax(pk, x); }
        double att_end;
        double att = smeter_att_scan(g, sm, {S.pw[cnt], p}, pk, att_end);    // attack average entering this thread's run
        AffMax dec = AffMax::identity();
        for (int j = 0; j < cnt; j++) {
            const double x = (double)run[j];
            att = ia * att + aa * x;
            dec = AffMax{id, da * x, att}.after(dec);
        }
        smeter_finish(g, sm, dec, att_end, pk);
    }
    if (t == 0) C.sm = sm;
}
hipError_t smeter_call_launch(const PcArgs &a, hipStream_t stream)
{
#ifdef PC_CENSUS
    if (a.layout_tag != PC_ARGS_TAG) return hipErrorInvalidValue;   // the caller's unit was compiled without the macro
#endif
    hipLaunchKernelGGL(smeter_call_kernel, dim3(a.channels), dim3(256), 0, stream, pc_traced(a));
    return hipGetLastError();
}

// =====================================================================================================
// The squelch half of CFmDemod (fmdemod.cpp:113-152), deferred out of the walk (PC_FM_DEFER).  None of it feeds
// back into the loop: the high-pass CFir over the audio, the average of its magnitude, the once-per-burst hysteresis
// decision and the CIir low-pass of the bursts that stay open are post-processing of the raw audio the walk leaves in
// the output rows -- a fifth of an FM tile's time in the sequential walk, a few microseconds as burst-parallel work:
//   1. fm_squelch_maps_kernel, one workgroup per (channel, burst): the burst's high-pass + |.| + average and its
//      low-pass, both from a ZERO start state, reduced to their affine maps (average: s -> A s + B; filter state:
//      s -> M s + v) -- the same scans the walk used, so the same words come out;
//   2. fm_squelch_decide_kernel, one workgroup per channel: the maps chained through the bursts in order (64 small
//      steps), the decision of every burst, the filter state each open burst starts from; the channel's state;
//   3. fm_squelch_apply_kernel, one workgroup per (channel, burst): zeros, or the low-pass from that start state.
// =====================================================================================================
// a tile's two maps (p: the squelch average, q: the low-pass state), as sq_and_lowpass builds them
template <int NW>
__device__ __forceinline__ Both<Aff1, Aff2> sq_lp_maps(const Wg<NW> &g, const float *sq, const float *x, int n, double a, double gn,
                                                       const double *apw, const PcIir &f, const double *tab)
{
    constexpr int LC = Wg<NW>::LC;
    const int base = g.base(), cnt = g.count(n);
    double p = 0.0, w1 = 0.0, w2 = 0.0;
#pragma unroll
    for (int j = 0; j < LC; j++) {
        const float sv = j < cnt ? sq[base + j] : 0.f;
        p = j < cnt ? a * p + gn * (double)sv : p;
        (void)biquad_chunk_step(f, j < cnt ? (double)x[base + j] : 0.0, j < cnt, w1, w2);
    }
    Both<Aff1, Aff2> m{{apw[cnt], p}, chunk_map2(tab, cnt, w1, w2)}, tot;
    g.scan(m, tot);
    return tot;
}

__global__ __launch_bounds__(256)
void fm_squelch_maps_kernel(PcArgs a)
{
    CSDR_WG_TRACE_SCOPE(a.trace, WGT_SQ_MAPS);
    using G = Wg<4>;
    constexpr int NT = G::NT, LC = G::LC;
    extern __shared__ __attribute__((aligned(16))) unsigned char pc_smem[];
    SqLds &S = *reinterpret_cast<SqLds *>(pc_smem);
    const PcBurstGroup bg = pc_burst_group(a.nbursts, a.sq_bpw);
    const int t = threadIdx.x, ch = bg.ch, b0 = bg.b0, b1 = bg.b1;
    if (a.out_rows && a.out_rows[ch] < 0) return;
    const PcChannel &C = a.chan[ch];
    if (C.mode != PC_MODE_FM) return;                    // uniform per workgroup
    const G g{t, t & 63, t >> 6, &S.sy};
    const PcRow row = PcRow::of(a, ch);
    const PcFir &fir = C.fm.hp;
    const int nt = fir.ntaps;
    stage_taps<NT>(S.h0, fir.coef, nt, t);
    for (int i = t; i < PT + PC_FIR_MAX + 17; i += NT) S.w0[i] = 0.f;
    pow_table(S.pw_sq, 1.0 - C.fm.sq_alpha, t);
    PcIir lp = C.fm.lp;
    biquad_table(S.bq, lp, t);
    g.sync();
    // the high-pass delay line at the start of this group's first burst: the audio in front of it (still raw: the apply
    // kernel runs after every maps workgroup has finished), the saved delay line in front of the call
    {
        const long g0 = (long)b0 * a.burst;
        for (int i = t; i < nt - 1; i += NT) {
            const long k = g0 - (nt - 1) + i;
            S.w0[i] = k >= 0 ? row.raw(k) : fir.zreal[i];   // (k < 0 only for burst 0: burst >= PC_FIR_MAX > ntaps - 1)
        }
    }
    float *au = S.w0 + (nt - 1);
    // the audio of the next tile is fetched while the current one goes through its filter and scan
    float nx[LC];
    const long first = (long)b0 * a.burst, end = (long)b1 * a.burst;
    auto fetch = [&](long p) {
#pragma unroll
        for (int j = 0; j < LC; j++) { const long i = p + t + NT * j; nx[j] = i < end ? row.raw(i) : 0.f; }
    };
    fetch(first);
    for (int b = b0; b < b1; b++) {
        const long g0 = (long)b * a.burst;
        Both<Aff1, Aff2> burst = Both<Aff1, Aff2>::identity();
        for (int t0 = 0; t0 < a.burst; t0 += PT) {
            const int n = (a.burst - t0) < PT ? (a.burst - t0) : PT;
#pragma unroll
            for (int j = 0; j < LC; j++) { const int i = t + NT * j; if (i < n) au[i] = nx[j]; }
            fetch(g0 + t0 + n);                          // bursts are contiguous: the next tile follows
            g.sync();
            float acc[LC];
            fir_blk<4>(S.h0, nt, S.w0, t, acc);
#pragma unroll
            for (int j = 0; j < LC; j++) S.w2[pc_out_index<4>(t, j) & (PT - 1)] = fabsf(acc[j]);
            g.sync();
            // this tile's maps behind what the burst has so far
            burst = sq_lp_maps(g, S.w2, au, n, 1.0 - C.fm.sq_alpha, C.fm.sq_alpha, S.pw_sq, lp, S.bq).after(burst);
            g.sync();
            slide(g, S.w0, nt - 1, n);                   // the next tile's / burst's delay line
            g.sync();
        }
        if (t == 0) burst.put(a.sqbuf + ((long)ch * a.nbursts + b) * PC_SQ_REC);
    }
}

__global__ __launch_bounds__(64)
void fm_squelch_decide_kernel(PcArgs a)
{
    CSDR_WG_TRACE_SCOPE(a.trace, WGT_SQ_DECIDE);
    const int t = threadIdx.x, ch = blockIdx.x;
    if (a.out_rows && a.out_rows[ch] < 0) return;
    PcChannel &C = a.chan[ch];
    if (C.mode != PC_MODE_FM) return;
    const PcRow row = PcRow::of(a, ch);
    PcFm &F = C.fm;
    // the high-pass delay line after the call: the last ntaps-1 raw audio samples (the apply kernel has not run yet)
    const int nt = F.hp.ntaps;
    const long total = (long)a.nbursts * a.burst;
    float keep = 0.f;
    if (t < nt - 1) {
        const long k = total - (nt - 1) + t;
        keep = k >= 0 ? row.raw(k) : F.hp.zreal[t + (int)total];
    }
    __syncthreads();
    if (t < nt - 1) F.hp.zreal[t] = keep;
    // the bursts' maps come in 64 at a time, one record per thread (a walk over global memory would pay a dependent
    // miss per burst); thread 0 chains them
    __shared__ double rec[64][8];
    __shared__ double res[64][3];
    double sq = F.sq_ave, w1 = F.lp.w1a, w2 = F.lp.w2a;
    int sqd = F.squelched;
    for (int c0 = 0; c0 < a.nbursts; c0 += 64) {
        const int cn = a.nbursts - c0 < 64 ? a.nbursts - c0 : 64;
        __syncthreads();
        if (t < cn) {
            const double *r = a.sqbuf + ((long)ch * a.nbursts + c0 + t) * PC_SQ_REC;
#pragma unroll
            for (int k = 0; k < 8; k++) rec[t][k] = r[k];
        }
        __syncthreads();
        if (t == 0) {
            for (int b = 0; b < cn; b++) {
                const double *r = rec[b];
                sq = r[0] * sq + r[1];
                sqd = squelch_decide(sq, F.sq_thresh, sqd);
                res[b][0] = (double)sqd; res[b][1] = w1; res[b][2] = w2;
                if (!sqd) {                                                     // the low-pass runs on open bursts only
                    const double nw1 = r[2] * w1 + r[3] * w2 + r[6], nw2 = r[4] * w1 + r[5] * w2 + r[7];
                    w1 = nw1; w2 = nw2;
                }
            }
        }
        __syncthreads();
        if (t < cn) {
            double *r = a.sqbuf + ((long)ch * a.nbursts + c0 + t) * PC_SQ_REC;
            r[8] = res[t][0]; r[9] = res[t][1]; r[10] = res[t][2];
        }
    }
    if (t == 0) { F.sq_ave = sq; F.squelched = sqd; F.lp.w1a = w1; F.lp.w2a = w2; }
}

__global__ __launch_bounds__(256)
void fm_squelch_apply_kernel(PcArgs a)
{
    CSDR_WG_TRACE_SCOPE(a.trace, WGT_SQ_APPLY);
    using G = Wg<4>;
    constexpr int NT = G::NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char pc_smem[];
    SqLds &S = *reinterpret_cast<SqLds *>(pc_smem);
    const PcBurstGroup bg = pc_burst_group(a.nbursts, a.sq_bpw);
    const int t = threadIdx.x, ch = bg.ch, b0 = bg.b0, b1 = bg.b1;
    if (a.out_rows && a.out_rows[ch] < 0) return;
    const PcChannel &C = a.chan[ch];
    if (C.mode != PC_MODE_FM) return;
    const G g{t, t & 63, t >> 6, &S.sy};
    const PcRow row = PcRow::of(a, ch);
    PcIir lp = C.fm.lp;
    biquad_table(S.bq, lp, t);
    g.sync();
    for (int b = b0; b < b1; b++) {
        const double *r = a.sqbuf + ((long)ch * a.nbursts + b) * PC_SQ_REC;
        const long g0 = (long)b * a.burst;
        if (r[8] != 0.0) {                               // squelched: zeros (fmdemod.cpp:139-143); uniform per workgroup
            for (int i = t; i < a.burst; i += NT) row.put(g0 + i, 0.f);
            continue;
        }
        lp.w1a = r[9]; lp.w2a = r[10];
        for (int t0 = 0; t0 < a.burst; t0 += PT) {
            const int n = (a.burst - t0) < PT ? (a.burst - t0) : PT;
            for (int i = t; i < n; i += NT) S.w2[i] = row.raw(g0 + t0 + i);
            g.sync();
            biquad_scan(g, S.w2, n, lp, S.bq);
            g.sync();
            for (int i = t; i < n; i += NT) row.put(g0 + t0 + i, S.w2[i]);
            g.sync();
        }
    }
}

hipError_t fm_squelch_launch(const PcArgs &a, hipStream_t stream)
{
#ifdef PC_CENSUS
    if (a.layout_tag != PC_ARGS_TAG) return hipErrorInvalidValue;   // the caller's unit was compiled without the macro
#endif
    static_assert(sizeof(SqLds) <= 20 * 1024, "eight squelch workgroups per CU");
    PcArgs b = a;
    b.sq_bpw = pc_bursts_per_wg(a);
    const int ngrp = pc_burst_groups(a.nbursts, b.sq_bpw);
    hipLaunchKernelGGL(fm_squelch_maps_kernel, dim3(a.channels * ngrp), dim3(256), sizeof(SqLds), stream, pc_traced(b));
    hipLaunchKernelGGL(fm_squelch_decide_kernel, dim3(a.channels), dim3(64), 0, stream, pc_traced(b));
    hipLaunchKernelGGL(fm_squelch_apply_kernel, dim3(a.channels * ngrp), dim3(256), sizeof(SqLds), stream, pc_traced(b));
    return hipGetLastError();
}

// stand-alone CFir / CIir objects (one lane each): op 0 FIR real, 1 FIR complex, 2 IIR real, 3 IIR complex
__global__ void filter_leaf_kernel(PcFir *fir, PcIir *iir, const float *in, float *out, int n, int op)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (op == 0) {
        for (int i = 0; i < n; i++) out[i] = fir_real(*fir, in[i]);
    } else if (op == 1) {
        for (int i = 0; i < n; i++) {
            float re = in[2 * i], im = in[2 * i + 1];
            fir_cpx(*fir, re, im);
            out[2 * i] = re; out[2 * i + 1] = im;
        }
    } else if (op == 2) {
        for (int i = 0; i < n; i++) out[i] = iir_a(*iir, in[i]);
    } else {
        for (int i = 0; i < n; i++) { out[2 * i] = iir_a(*iir, in[2 * i]); out[2 * i + 1] = iir_b(*iir, in[2 * i + 1]); }
    }
}

hipError_t filter_leaf_launch(PcFir *fir, PcIir *iir, const float *in, float *out, int n, int op, hipStream_t stream)
{
    hipLaunchKernelGGL(filter_leaf_kernel, dim3(1), dim3(64), 0, stream, fir, iir, in, out, n, op);
    return hipGetLastError();
}

// CSMeter::GetAve / GetPeak (dsp/smeter.cpp:98-112) of every channel of a unit at once, without moving the
// channel state: ave[row] = average + 5 dB, peak[row] = peak + 5 dB and the peak is reset to 0 as GetPeak
// does.  rows: optional output index of each channel.
template <class T>
__global__ void smeter_collect_kernel(PcChannel *chan, int channels, const int *rows, T *ave, T *peak)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= channels) return;
    const int o = rows ? rows[c] : c;
    if (o < 0) return;                  // a row whose receiver has moved to another plan group (csdr_demod_batch_set_demod)
    if (ave) ave[o] = (T)(chan[c].sm.ave_mag + refc::SM_CALIBRATION);
    if (peak) {
        peak[o] = (T)(chan[c].sm.peak_mag + refc::SM_CALIBRATION);
        chan[c].sm.peak_mag = 0.0;
    }
}
hipError_t smeter_collect_launch(PcChannel *chan, int channels, const int *rows, float *ave, float *peak, hipStream_t stream)
{
    hipLaunchKernelGGL(smeter_collect_kernel<float>, dim3((channels + 255) / 256), dim3(256), 0, stream, chan, channels, rows, ave, peak);
    return hipGetLastError();
}
hipError_t smeter_collect_launch(PcChannel *chan, int channels, const int *rows, double *ave, double *peak, hipStream_t stream)
{
    hipLaunchKernelGGL(smeter_collect_kernel<double>, dim3((channels + 255) / 256), dim3(256), 0, stream, chan, channels, rows, ave, peak);
    return hipGetLastError();
}

template <int NW, bool LEAN>
static hipError_t pc_launch_nw(const PcArgs &a, hipStream_t stream)
{
    // once per device and instantiation (the attribute belongs to the device, and a process may drive several)
    if (sizeof(PcLds) > 64 * 1024) {
        hipError_t e = CSDR_MAX_LDS_ONCE((&postchain_kernel<NW, LEAN>), sizeof(PcLds));
        if (e != hipSuccess) return e;
    }
#ifdef PC_CENSUS
    {   // this walk's place in the census buffer: channels x tiles records behind those of the walks before it
        PcCensusHost &h = pc_census_host();
        const int tiles = a.nbursts * ((a.burst + PT - 1) / PT);
        PcArgs b = a;
        b.census = PcCensusArg{h.buf, h.next, tiles, h.tiles, h.launches + 1, NW | (LEAN ? 1 : 0) << 8, 0};
        if (h.buf) { h.next += a.channels * tiles; h.tiles += tiles; h.launches++; }
        hipLaunchKernelGGL((postchain_kernel<NW, LEAN>), dim3(a.channels), dim3(64 * NW), sizeof(PcLds), stream, pc_traced(b));
        return hipGetLastError();
    }
#endif
    hipLaunchKernelGGL((postchain_kernel<NW, LEAN>), dim3(a.channels), dim3(64 * NW), sizeof(PcLds), stream, pc_traced(a));
    return hipGetLastError();
}
hipError_t postchain_launch(const PcArgs &a, hipStream_t stream)
{
#ifdef PC_CENSUS
    if (a.layout_tag != PC_ARGS_TAG) return hipErrorInvalidValue;   // the caller's unit was compiled without the macro
#endif
    // waves per channel: four when the channels alone cannot fill the chip, else one; CSDR_POSTCHAIN_WAVES=1|4 overrides
    static int forced = -1;
    if (forced < 0) { const char *env = getenv("CSDR_POSTCHAIN_WAVES"); forced = env ? atoi(env) : 0; }
    int nw = a.channels <= 1024 ? 4 : 1;
    if (forced == 1 || forced == 4) nw = forced;
    // the lean walk (four waves): no S-meter in the launch, AGC peaks precomputed for every receiver that has the AGC
    // on, the squelch of every FM receiver deferred -- the caller (PcUnit::run) says so with PC_LEAN
    static const bool lean_ok = !(getenv("CSDR_PC_LEAN") && atoi(getenv("CSDR_PC_LEAN")) == 0);
    if (nw == 4 && (a.flags & PC_LEAN) && lean_ok) return pc_launch_nw<4, true>(a, stream);
    return nw == 4 ? pc_launch_nw<4, false>(a, stream) : pc_launch_nw<1, false>(a, stream);
}

}  // namespace csdr
