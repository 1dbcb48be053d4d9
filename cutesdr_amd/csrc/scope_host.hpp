// scope_host.hpp -- the batch test-bench scope's arithmetic that host and device share (reference gui/testbench.cpp:
// DisplayData's time branch :613-635 / :673-694, ChkForTrigger :819-898, Reset :541-548, :574, the slots :247-299).
//
// The emission rule is stateless: a sample with input position i emits screen pixels while (double)i / samplerate >=
// (double)pos * pixel time (:618-621), pos runs 0..w-1 and at w both positions go back to 0 (:627-632).  So pixel p of
// a sweep that starts at input position 0 is emitted by sample k(p) = the first i with (double)i / sr >= (double)p *
// pix, a sweep consumes k(w-1) + 1 samples, and the screen position of an emission is its number since the last reset
// modulo w.  A sweep that is entered in the middle (state inpos, pos; possibly with a pixel time changed since by
// OnHorzSpan) emits pixel p at input position max(k(p), inpos).  k(p) is taken from ceil(p * pix * sr) and corrected
// with the reference's own fp64 comparison, so it is the reference's index whatever that product rounds to.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>

namespace csdr {
namespace sc {

constexpr int kMaxW = 2048;                              // TB_MAX_SCREENSIZE (gui/testbench.h:46)
constexpr double kMaxSweep = 1073741824.0;               // samples of one sweep: m_TimeInPos is an int
enum { TRIG_OFF = 0, TRIG_PNORM = 1, TRIG_PSINGLE = 2, TRIG_NNORM = 3, TRIG_NSINGLE = 4 };
enum { ST_WAIT = 0, ST_CAPTURE = 1, ST_DISPLAY = 2, ST_WAITDISPLAY = 3 };
enum { F_RESET = 1, F_REARM = 2 };

// (int) of a sample (:623-625): saturating, NaN gives 0 (the reference's conversion is undefined there)
__host__ __device__ inline int sat_int(double x)
{
    if (!(x == x)) return 0;
    if (x >= 2147483647.0) return INT_MAX;
    if (x <= -2147483648.0) return INT_MIN;
    return (int)x;
}

// the first input position i >= 0 with (double)i / sr >= (double)p * pix (:618-621)
__host__ __device__ inline long long first_index(int p, double pix, double sr)
{
    const double t = (double)p * pix;
    if (!(t > 0.0)) return 0;
    const double c = ceil(t * sr);
    long long i = c < 2.0 * kMaxSweep ? (long long)c : (long long)(2.0 * kMaxSweep);
    while (i > 0 && (double)(i - 1) / sr >= t) i--;
    while ((double)i / sr < t) i++;
    return i;
}

// One call of one receiver: where its emissions fall.  Emission e (0-based within the call) has the global pixel
// number g = pos0 + e, sweep g / w and pixel g % w; sweep 0 is the one the call enters at (inpos0, pos0).
struct Plan {
    double pix, sr;
    int w, pos0;
    long long inpos0;
    long long first;                     // samples of the call that sweep 0 consumes (may exceed n)
    long long len;                       // k(w-1) + 1: samples of a whole sweep
    long long emits;                     // emissions of the call
    int pos_end;                         // m_TimeScrnPos after the call
    long long inpos_end;                 // m_TimeInPos after the call

    // index within the call of the sample that emits e
    __host__ __device__ long long sample(long long e) const
    {
        const long long g = (long long)pos0 + e, m = g / w;
        const long long k = first_index((int)(g % w), pix, sr);
        if (m == 0) return k > inpos0 ? k - inpos0 : 0;
        return first + (m - 1) * len + k;
    }
    // pixels p in [lo, w) emitted by the first `avail` samples of a sweep entered at input position `in`
    __host__ __device__ int count(int lo, long long in, long long avail) const
    {
        int a = lo, b = w;                               // first p in [lo, w) whose sample index is >= avail
        while (a < b) {
            const int mid = (a + b) >> 1;
            const long long k = first_index(mid, pix, sr);
            if ((k > in ? k - in : 0) >= avail) b = mid; else a = mid + 1;
        }
        return a - lo;
    }
};

__host__ __device__ inline Plan make_plan(long long inpos0, int pos0, double pix, double sr, int w, long long n)
{
    Plan p;
    p.pix = pix; p.sr = sr; p.w = w; p.pos0 = pos0; p.inpos0 = inpos0;
    const long long kl = first_index(w - 1, pix, sr);
    p.len = kl + 1;
    p.first = (kl > inpos0 ? kl - inpos0 : 0) + 1;
    if (p.first > n) {                                   // the call ends inside the sweep it entered
        p.emits = p.count(pos0, inpos0, n);
        p.pos_end = pos0 + (int)p.emits;
        p.inpos_end = inpos0 + n;
    } else {
        const long long rest = n - p.first, full = rest / p.len, rem = rest % p.len;
        const int c = p.count(0, 0, rem);
        p.emits = (long long)(w - pos0) + full * w + c;
        p.pos_end = c;
        p.inpos_end = rem;
    }
    return p;
}

// m_DisplaySkipValue as Reset, OnDisplayRate and OnHorzSpan compute it (:252-253, :276-277, :564-565).  The member
// is a qint32 (gui/testbench.h:174), so the quotient is truncated when it is stored.
inline int skip_value(int span_ms, int display_rate, double sr)
{
    const double capturesize = ((double)span_ms * sr / 1000.0);
    return sat_int(sr / (capturesize * display_rate));
}
// m_TimeScrnPixel (:278, :541)
inline double pixel_time(int span_ms, int w) { return .001 * (double)((double)span_ms / (double)w); }

// TRIG_OFF (:823-834): m sweep starts seen with the counter at cnt: the displays among them, the 1-based number of
// the last displaying start, and the counter afterwards.  ++cnt >= skip && cnt > 2 is cnt >= max(skip, 3) on ints.
struct FreeRun { long long displays, last; long long cnt; };
__host__ __device__ inline FreeRun free_run(long long cnt, int skip, long long m)
{
    const long long T = skip > 3 ? skip : 3;
    const long long f = T - cnt > 1 ? T - cnt : 1;       // the first start that displays
    FreeRun r;
    if (m < f) { r.displays = 0; r.last = 0; r.cnt = cnt + m; return r; }
    r.displays = 1 + (m - f) / T;
    r.last = f + (r.displays - 1) * T;
    r.cnt = m - r.last;
    return r;
}

// what a put hands to the kernel per receiver (host, one pinned slot per launch)
struct ChanParam {
    double pix, sr;
    int n, skip, level, mode, flags, vert;
};

// data-dependent state of one receiver, on the device
struct ChanState {
    long long inpos;                     // m_TimeInPos
    int pos;                             // m_TimeScrnPos
    int prev;                            // m_PreviousSample
    int trigstate, trigcounter, trigbufpos;
    int skipcounter;                     // m_DisplaySkipCounter
    unsigned emits;                      // NewTimeData emits since creation (modulo 2^32)
    int pad;
};

// A reset and the re-arm that travel with a put (Reset :544-548, :574 -- the caller clears the ring; DrawTimePlot :995-999)
__host__ __device__ inline void apply_flags(ChanState &st, int flags)
{
    if (flags & F_RESET) { st.inpos = 0; st.pos = 0; st.prev = 0; st.trigstate = ST_WAIT; st.skipcounter = -2; }
    if (flags & F_REARM) st.trigstate = ST_WAIT;         // the host leaves the single modes out
}
// true when ChkForTrigger looks for a crossing in this call (:837, :858)
__host__ __device__ inline bool searches(const ChanState &st, const ChanParam &par)
{
    return par.mode >= TRIG_PNORM && par.mode <= TRIG_NSINGLE && st.trigstate == ST_WAIT;
}
__host__ __device__ inline bool crossing(int mode, int level, int cur, int prv)             // :840, :861
{
    return (mode == TRIG_PNORM || mode == TRIG_PSINGLE) ? (cur >= level && prv < level) : (cur <= level && prv > level);
}
// ChkForTrigger over the E emissions of a call without the data: `trig` is the first crossing among them (-1: none;
// only looked at when searches()).  Brings the trigger members of st up to date and returns the emission of the call
// whose check copies the screen out (-1: none) and the ring slot the copy starts from relative to that emission's own
// slot (rot).  In the triggered modes a trigger at emission t displays at t + max(Post, 1): ++m_TrigCounter >= Post is
// looked at from the emission after the trigger (:847-854).
struct Display { long long at; int rot; };
__host__ __device__ inline Display decide(ChanState &st, const ChanParam &par, int w, long long E, long long trig)
{
    const int pos0 = st.pos, post = (7 * w) / 10;
    const int delay = post > 1 ? post : 1;
    Display d = {-1, 0};
    if (par.mode == TRIG_OFF) {                          // :823-834: decided at screen position 0
        const long long e0 = (w - pos0) % w;             // the first emission at position 0
        const long long starts = E > e0 ? (E - e0 + w - 1) / w : 0;
        const FreeRun fr = free_run(st.skipcounter, par.skip, starts);
        st.skipcounter = (int)fr.cnt;
        if (fr.displays) {
            d.at = e0 + (fr.last - 1) * w; d.rot = post;
            st.trigbufpos = 0; st.trigstate = ST_WAITDISPLAY; st.emits += (unsigned)fr.displays;
        }
    } else if (par.mode >= TRIG_PNORM && par.mode <= TRIG_NSINGLE) {
        if (st.trigstate == ST_WAIT) {
            if (trig >= 0) {
                st.trigbufpos = (int)((pos0 + trig) % w);
                st.trigcounter = 0;
                if (trig + delay < E) d.at = trig + delay;
                else { st.trigstate = ST_CAPTURE; st.trigcounter = (int)(E - 1 - trig); }
            }
        } else if (st.trigstate == ST_CAPTURE) {
            const long long k = (long long)delay - st.trigcounter > 1 ? (long long)delay - st.trigcounter : 1;
            if (k - 1 < E) d.at = k - 1;
            else st.trigcounter += (int)E;
        }
        if (d.at >= 0) { st.trigstate = ST_WAITDISPLAY; st.trigcounter = 0; st.emits += 1u; }
    }
    return d;
}
// screen entry i of a display (:884-894): the emission of the call it is (>= 0), or, for an emission before the call
// (< 0, at least -w), the slot of the carried ring that holds it
__host__ __device__ inline long long screen_source(const Display &d, int i, int w, int pos0, int *slot)
{
    int j = d.rot + i; if (j >= w) j -= w;
    const long long e = d.at - w + j;
    if (e < 0) { int k = (int)((pos0 + e) % w); *slot = k < 0 ? k + w : k; }
    return e;
}

// one receiver's settings on the host: the slots' members
struct Chan {
    int rate = 10, span = 100, vert = 65000, level = 100, mode = TRIG_OFF;      // constructor, :111-117
    double sr = 1.0;                                                            // m_DisplaySampleRate, :102
    double pix = 0.0;
    int skip = 0;
    int flags = 0;                                                              // applied by the next put, in stream order
    unsigned seen = 0;                                                          // emits already reported by get_emits

    void derive(int w) { skip = skip_value(span, rate, sr); pix = pixel_time(span, w); }
    void on_display_rate(int r) { rate = r; skip = skip_value(span, rate, sr); }                // :247-254
    void on_horz_span(int s, int w) { span = s; skip = skip_value(span, rate, sr); pix = pixel_time(span, w); }    // :270-279
    void reset(int w) { derive(w); flags |= F_RESET; }                                          // :541-548, :555-565, :574
    void on_trigger_mode(int m, int w) { mode = m; reset(w); }                                  // :288-292
    void time_plot_done() { if (mode != TRIG_PSINGLE && mode != TRIG_NSINGLE) flags |= F_REARM; }   // :995-999
    // the settings of one put of n samples at rate fs; takes the pending flags with it
    void prepare(int n, double fs, int w, ChanParam &p)
    {
        p.n = n;
        if (n > 0 && sr != fs) { sr = fs; reset(w); p.n = 0; }      // :587-592: reset, and the call's samples are not used
        p.pix = pix; p.sr = sr; p.skip = skip; p.level = level; p.mode = mode; p.vert = vert;
        p.flags = flags;
        flags = 0;
    }
};

}  // namespace sc
}  // namespace csdr
