// testgen_host.hpp -- host state machine of the batch signal generator (CTestBench's sweep / pulse generator,
// reference gui/testbench.cpp:352-517): everything that decides an integer -- the frequency sequence, the end of the
// sweep, the pulse gate -- reproduced bit for bit without walking the samples, and the phase as an exact 128-bit sum.
//
// The reference carries "x <- fl(x + d) until x crosses a limit" twice (sweep frequency, pulse timer).  Inside one
// binade every partial sum is a multiple of the binade's ulp, so fl(x + d) - x is one constant, exactly representable
// step e; the one exception, d's remainder being exactly half an ulp, alternates only while x's mantissa is odd and
// is constant (the even multiple) after one literal step.  plan_run() returns that step and how many additions it
// is good for (to the binade's end or the limit, less two for safety); everything else is walked one literal
// addition at a time.  Cost: O(binades crossed).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

namespace csdr {
namespace tg {

typedef unsigned __int128 u128;

static const uint64_t kForever = ~0ull;

struct Run {
    double e;            // exact step: x_k = x + k * e for k = 0..m, as the literal additions give it
    uint64_t m;          // additions covered (0: take a literal step); none of x_1..x_m crosses the limit
};

// x: current value, d: the constant added, limit/strict: stop rule (x > limit when strict, x >= limit otherwise)
inline Run plan_run(double x, double d, double limit, bool strict)
{
    Run r = {0.0, 0};
    if (d == 0.0) { r.m = kForever; return r; }
    const double g = x + d;
    if (g == x) { r.m = kForever; return r; }            // d is absorbed: x never moves again
    if (x == 0.0 || !std::isfinite(g) || std::fabs(x) < std::numeric_limits<double>::min()) return r;
    int ex, eg;
    (void)std::frexp(x, &ex);
    (void)std::frexp(g, &eg);
    if (ex != eg || (x < 0) != (g < 0)) return r;       // the step leaves the binade: literal
    const double e = g - x;                              // exact: both are multiples of the binade's ulp
    const double ulp = std::ldexp(1.0, ex - 53);
    if (std::fabs(d - e) == 0.5 * ulp && std::fmod(std::fabs(x) / ulp, 2.0) != 0.0) return r;   // tie on an odd mantissa
    const double lo = std::ldexp(1.0, ex - 1), hi = std::ldexp(1.0, ex);                         // |x| in [lo, hi)
    double kb, kt = 1e300;
    if ((e > 0) == (x > 0)) kb = std::floor((hi - std::fabs(x)) / std::fabs(e));                 // magnitude grows
    else kb = std::floor((std::fabs(x) - lo) / std::fabs(e));
    if (e > 0) {
        const bool crossed = strict ? x > limit : x >= limit;
        if (crossed || std::isnan(limit)) return r;
        if (limit < 1e300) kt = std::floor((limit - x) / e);
    } else if (strict ? g > limit : g >= limit) return r;                 // falling but still across: the next sum says so
    double k = (kb < kt ? kb : kt) - 2.0;
    if (!(k >= 1.0)) return r;
    r.e = e;
    r.m = k > 9e18 ? (uint64_t)9e18 : (uint64_t)k;
    return r;
}

// first index i >= 1 with x_i > limit (strict) or x_i >= limit, x_0 = x0, x_i = fl(x_{i-1} + d); the value there.
// kForever when the sequence never gets there (d <= 0 below the limit, or d absorbed); value = where it ends up or 0.
inline uint64_t first_crossing(double x0, double d, double limit, bool strict, double *value)
{
    double x = x0;
    uint64_t i = 0;
    if (!(d > 0.0)) {                                    // never rising: the first addition decides
        x += d;
        if (value) *value = x;
        return (strict ? x > limit : x >= limit) ? 1 : kForever;
    }
    for (;;) {
        const Run r = plan_run(x, d, limit, strict);
        if (r.m == kForever) { if (value) *value = x; return kForever; }
        if (r.m > 0) { x += (double)r.m * r.e; i += r.m; continue; }      // exact: a multiple of the ulp in the binade
        x += d; i++;
        if ((strict ? x > limit : x >= limit) || std::isnan(x)) { if (value) *value = x; return std::isnan(x) ? kForever : i; }
    }
}

// x_i of the same sequence with no stop rule
inline double value_at(double x0, double d, uint64_t index)
{
    double x = x0;
    uint64_t i = 0;
    while (i < index) {
        const Run r = plan_run(x, d, std::numeric_limits<double>::infinity(), false);
        if (r.m == kForever) return x;
        if (r.m > 0) { const uint64_t k = r.m < index - i ? r.m : index - i; x += (double)k * r.e; i += k; continue; }
        x += d; i++;
    }
    return x;
}

// v turns -> 128-bit fixed point (2^128 = one turn), two's complement, modulo one turn; 64-bit mantissa arithmetic
inline u128 turns_u128(long double v)
{
    const bool neg = v < 0;
    long double a = neg ? -v : v;
    if (!(a < 1.8e19L)) return 0;                        // (not a frequency anybody sets)
    a -= floorl(a);
    long double t = ldexpl(a, 64);
    const uint64_t hi = (uint64_t)t;
    t = ldexpl(t - (long double)hi, 64);
    const uint64_t lo = (uint64_t)t;
    const u128 u = ((u128)hi << 64) | lo;
    return neg ? (u128)0 - u : u;
}

static const int kMaxSeg = 8;                            // phase segments one launch takes per receiver

// what one launch needs of one receiver (testgen_kernels.hip); phase in 128-bit turns as lo/hi words
struct ChanParam {
    uint64_t seg_p[kMaxSeg][2];      // phase at the segment's first sample
    uint64_t seg_d[kMaxSeg][2];      // phase increment there
    uint64_t seg_d2[kMaxSeg][2];     // its step per sample
    uint32_t seg_start[kMaxSeg];     // first sample of the segment, counted from the call's first sample
    uint32_t nseg;                   // 0: nothing to do in this launch (generator off: the row is left alone)
    uint32_t gate_on;                // pulse modulation active (width > 0)
    uint32_t j_lo, j_hi;             // the launch writes samples j_lo <= j < j_hi of the call
    uint64_t pos0;                   // pulse timer index before the launch's first sample
    uint64_t wrap1;                  // additions until the timer first restarts
    uint64_t period;                 // K: additions per period
    uint64_t width;                  // W: timer indices 0..W-1 are ON
    uint64_t noise_key;              // per-receiver key of the noise draws
    uint64_t count0;                 // noise sample counter of the call's first sample
    uint64_t noise_on;               // noise power > -160 dB
    double amp, noise_amp;
    uint64_t pad_;
};
static_assert(sizeof(ChanParam) % 16 == 0, "rows of ChanParam stay 16-byte aligned");

inline uint64_t mix64(uint64_t z)                        // SplitMix64's finaliser
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static const uint64_t kGolden = 0x9E3779B97F4A7C15ull;
inline uint64_t noise_key(uint64_t seed, int channel) { return mix64(seed + kGolden * (uint64_t)(channel + 1)); }

// One CTestBench generator.  Members named after the reference's.
struct Gen {
    bool on = false;
    double start = 0.0, stop = 0.0, rate = 0.0;         // Hz, Hz, Hz/s
    double fs = 1.0;                                     // m_GenSampleRate
    double freq = 0.0, inc = 0.0;                        // m_SweepFrequency at the run's start, m_SweepRateInc
    double width = 0.01, period = 0.5;                   // seconds
    double sig_db = 0.0, noise_db = -160.0, amp = 32767.0, noise_amp = 32767.0e-8;
    uint64_t timer = 0;                                  // m_PulseTimer as the index of its partial sum
    uint64_t count = 0;                                  // samples generated since creation / set_seed
    u128 phase = 0;                                      // m_SweepAcc in turns, exact
    // current run of the frequency: f_k = freq + k * run.e, k = run_k now
    Run run = {0.0, 0};
    uint64_t run_k = 0;
    bool run_valid = false;
    u128 run_d = 0, run_d2 = 0;                          // phase increment at the run's start, its step
    // pulse pattern, a function of (fs, period, width)
    bool pulse_valid = false;
    uint64_t K = 1, W = 1;

    double freq_now() const { return run_valid ? freq + (double)run_k * run.e : freq; }
    void drop_run() { freq = freq_now(); run_valid = false; run_k = 0; }
    void set_amps()
    {
        amp = 32767.0 * std::pow(10.0, sig_db / 20.0);
        noise_amp = 32767.0 * std::pow(10.0, noise_db / 20.0);
    }
    void reset()                                         // the generator part of CTestBench::Reset()
    {
        run_valid = false; run_k = 0;
        freq = start; phase = 0; inc = rate / fs;
        set_amps();
        timer = 0;
    }
    void on_sweep_start(double hz) { start = hz; run_valid = false; run_k = 0; freq = start; phase = 0; }
    void on_sweep_stop(double hz) { stop = hz; run_valid = false; run_k = 0; freq = start; phase = 0; }
    void on_sweep_rate(double hz_s) { drop_run(); rate = hz_s; phase = 0; inc = rate / fs; }
    void on_pulse_width(double s) { width = s; pulse_valid = false; }
    void on_pulse_period(double s) { period = s; pulse_valid = false; }
    void on_signal_pwr(double db) { sig_db = db; amp = 32767.0 * std::pow(10.0, sig_db / 20.0); }
    void on_noise_pwr(double db) { noise_db = db; noise_amp = 32767.0 * std::pow(10.0, noise_db / 20.0); }

    void pulse_pattern()
    {
        if (pulse_valid) return;
        const double d = 1.0 / fs;
        K = first_crossing(0.0, d, period, true, nullptr);
        W = first_crossing(0.0, d, width, true, nullptr);
        pulse_valid = true;
    }
    static bool same_binade(double a, double b)
    {
        int ea, eb;
        (void)std::frexp(a, &ea);
        (void)std::frexp(b, &eb);
        return a != 0.0 && b != 0.0 && ea == eb && (a < 0) == (b < 0) && std::isfinite(a) && std::isfinite(b);
    }
    void start_run()
    {
        run = plan_run(freq, inc, stop, false);
        if (run.m == 0 && same_binade(freq, freq + inc)) run.e = (freq + inc) - freq;   // exact; lets the run grow below
        run_k = 0; run_valid = true;
        run_d = turns_u128((long double)freq / (long double)fs);
        run_d2 = turns_u128((long double)run.e / (long double)fs);
    }
    // Up to n samples of one launch into p (appending segments from sample j0); returns how many it took: fewer than
    // n when the launch's segment table is full.  The state advances by exactly that many samples.  A segment is one
    // run of the frequency (or what is left of it at the call's first sample).
    uint32_t advance(uint32_t j0, uint32_t n, ChanParam &p)
    {
        uint32_t done = 0;
        bool open = false;                               // the current run already has its segment in p
        while (done < n) {
            if (!run_valid) { start_run(); open = false; }
            if (!open) {
                if (p.nseg == (uint32_t)kMaxSeg) break;
                const u128 d = run_d + run_d2 * (u128)run_k;
                const uint32_t s = p.nseg++;
                p.seg_start[s] = j0 + done;
                p.seg_p[s][0] = (uint64_t)phase; p.seg_p[s][1] = (uint64_t)(phase >> 64);
                p.seg_d[s][0] = (uint64_t)d; p.seg_d[s][1] = (uint64_t)(d >> 64);
                p.seg_d2[s][0] = (uint64_t)run_d2; p.seg_d2[s][1] = (uint64_t)(run_d2 >> 64);
                open = true;
            }
            const uint64_t left = run.m == kForever ? kForever : run.m + 1 - run_k;        // samples the run still has
            const uint32_t take = left < (uint64_t)(n - done) ? (uint32_t)left : n - done;
            const u128 d = run_d + run_d2 * (u128)run_k, t = (u128)take;
            phase += d * t + run_d2 * (t * (t - 1) / 2);
            run_k += take; done += take;
            if (run.m != kForever && run_k == run.m + 1) {                // the literal addition behind the run
                const double x = freq + (double)run.m * run.e, g = x + inc;
                if (!(g >= stop) && run.e != 0.0 && same_binade(x, g) && g - x == run.e) { run.m++; continue; }   // the run goes on
                freq = g;
                if (freq >= stop) inc = 0.0;
                run_valid = false; run_k = 0;
            }
        }
        return done;
    }
    // pulse timer over `take` samples: the words of the launch, then the new index
    void pulse(uint32_t take, ChanParam &p)
    {
        p.gate_on = width > 0.0;
        if (!p.gate_on) { p.pos0 = 0; p.wrap1 = kForever; p.period = 1; p.width = 1; return; }
        pulse_pattern();
        p.pos0 = timer; p.period = K; p.width = W;
        p.wrap1 = timer + 1 >= K ? 1 : K - timer;
        const uint64_t m = take;
        timer = m < p.wrap1 ? timer + m : (K == kForever ? m - p.wrap1 : (m - p.wrap1) % K);
    }
};

}  // namespace tg
}  // namespace csdr
