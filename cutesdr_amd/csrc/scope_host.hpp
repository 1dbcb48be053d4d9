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
//
// The FFT view (DisplayData's frequency branch :594-611 / :654-672, DrawFftPlot :1005-1068) has no data-dependent frame
// logic at all: given m_FftBufPos, the skip counter, the skip value and n, the frames of a call that reach
// PutInDisplayFFT are an arithmetic progression (fft_plan), sample i of such a frame lies in the carried partial
// frame or in the call's row (fft_source), and the bels -> pixel mapping of GetScreenIntegerFFTData (dsp/fft.cpp:
// 308-410) is a pure function of a few integers (make_fft_map, fft_pixel).  The host keeps position and counter of an
// FFT-view receiver itself (sc::Chan) and hands the kernel the progression.
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
enum { F_RESET = 1, F_REARM = 2, F_PEAK = 4 };         // F_PEAK: OnEnablePeak's clearing (:334-343)
enum { VIEW_TIME = 0, VIEW_FFT = 1 };
constexpr int kFftN = 2048;                              // TEST_FFTSIZE
constexpr double kFftMaxRate = 2147483632.0;             // an FFT-view receiver: (qint32)fs and the + 5 of :537-538 stay in an int
constexpr double kFftMaxdB = 10.0, kFftMindB = -170.0;   // m_MaxdB (:96) and m_MaxdB - TB_VERT_DIVS (18) * m_dBStepSize (:98, :1257)

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

// ---- the FFT view
// m_DisplaySkipValue as Reset and OnDisplayRate compute it in this view (:257, :570), truncated into the qint32
inline int fft_skip_value(int display_rate, double sr) { return sat_int(sr / (double)((long long)kFftN * display_rate)); }
// m_Span (:537-538): (qint32)fs, then rounded to a multiple of ten with C's remainder; sr < kFftMaxRate
inline int fft_span(double sr)
{
    const int s = sat_int(sr);
    return s - (s + 5) % 10 + 5;
}
// The frames that complete in a call of n samples entered at m_FftBufPos = pos with the skip counter at cnt (:597-610):
// frame j (0-based among them) is used when `++cnt >= skip` holds at its end.  The counter goes back to 0 at a used
// frame, so the used ones are first, first + step, ... (count of them); pos_end and cnt_end are the members afterwards.
struct FftPlan { long long frames, first, step, count, cnt_end; int pos_end; };
__host__ __device__ inline FftPlan fft_plan(int pos, long long cnt, int skip, long long n)
{
    FftPlan p;
    const long long avail = (long long)pos + n;
    p.frames = avail / kFftN;
    p.pos_end = (int)(avail - p.frames * kFftN);
    p.step = skip > 1 ? skip : 1;
    const long long m = (long long)skip - cnt > 1 ? (long long)skip - cnt : 1;   // the first increment that reaches skip
    p.first = m - 1;
    if (p.frames > p.first) {
        p.count = (p.frames - 1 - p.first) / p.step + 1;
        p.cnt_end = p.frames - 1 - (p.first + (p.count - 1) * p.step);
    } else {
        p.count = 0;
        p.cnt_end = cnt + p.frames;
    }
    return p;
}
// sample i of completing frame j of a call entered with `fill` carried samples: its index in the carry (the return
// value is < 0: index + fill) or in the call's row (>= 0)
__host__ __device__ inline long long fft_source(long long j, int i, int fill) { return j * kFftN + i - fill; }

// GetScreenIntegerFFTData's integers (dsp/fft.cpp:323-345) for DrawFftPlot's call (:1026-1043): start = -m_Span/2 for a
// frame completed by a complex put, else 0, stop = m_Span/2 (C's division), fs the rate of the last Reset
struct FftMap { int bin_min, bin_max, bins, h; double gain, off; };   // bins: the "more FFT points than plot points" branch
__host__ __device__ inline FftMap make_fft_map(int span, int cpx, double fs, int w, int h)
{
    FftMap m;
    const int start = cpx ? -span / 2 : 0, stop = span / 2, maxbin = kFftN - 1;
    m.bin_min = sat_int((double)start * (double)kFftN / fs) + kFftN / 2;
    m.bin_max = sat_int((double)stop * (double)kFftN / fs) + kFftN / 2;
    if (m.bin_min < 0) m.bin_min = 0;
    if (m.bin_min >= maxbin) m.bin_min = maxbin;
    if (m.bin_max < 0) m.bin_max = 0;
    if (m.bin_max >= maxbin) m.bin_max = maxbin;
    m.bins = (m.bin_max - m.bin_min) > w;
    m.h = h;
    m.off = kFftMaxdB / 10.0;
    m.gain = -10.0 / (kFftMaxdB - kFftMindB);
    return m;
}
__host__ __device__ inline int fft_level(const FftMap &m, double bel)                        // fft.cpp:369-373
{
    const int y = sat_int((double)m.h * m.gain * (bel - m.off));
    return y < 0 ? 0 : (y > m.h ? m.h : y);
}
// pixel x < w of the screen; bel(i) is m_pFFTAveBuf[i] as a double.  In the bins branch a pixel shows the smallest y of
// the bins i with ((i - bin_min) * w) / (bin_max - bin_min) == x (:364-389: x never decreases along i, so "first bin of
// a pixel sets it, a smaller one replaces it" is that minimum); those bins are d = i - bin_min in
// [ceil(x r / w), ceil((x + 1) r / w) - 1], r = bin_max - bin_min > w: never empty.  Bin bin_max maps to x = w, which
// the reference writes past the screen (OutBuf[w]); it is dropped.  Else pixel x shows bin bin_min + (x r) / w (:394-406).
template <class B> __host__ __device__ inline int fft_pixel(const FftMap &m, int w, int x, B bel)
{
    const int r = m.bin_max - m.bin_min;
    if (!m.bins) return fft_level(m, bel(m.bin_min + (x * r) / w));
    const int lo = (x * r + w - 1) / w, hi = ((x + 1) * r + w - 1) / w - 1;
    int y = INT_MAX;
    for (int d = lo; d <= hi; d++) { const int v = fft_level(m, bel(m.bin_min + d)); y = v < y ? v : y; }
    return y;
}

// what a put hands to the kernel per receiver (host, one pinned slot per launch)
struct ChanParam {
    double pix, sr;
    int n, skip, level, mode, flags, vert;
    // the FFT view (view == VIEW_FFT): the call's used frames first, first + step, ... (count) among the `frames` that
    // complete, entered with `fill` samples in carry buffer `cur`; position and counter afterwards; the mapping
    int view, h;
    int fill, cur, frames, first, step, count, pos_end, cnt_end;
    FftMap map;
};

// what the FFT view keeps on the device per receiver beside carries, bels, screen and peak
struct FftState {
    int pos;                             // m_FftBufPos
    int total;                           // CFft::m_TotalCount since the last Reset
    int cpx;                             // the last drawn frame was mapped as complex (m_CurrentDataIsCpx at that draw)
    int pad;
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
    int view = VIEW_TIME;                // m_TimeDisplay (deviation: the constructor's default is the FFT view, :110)
    int peak_on = 0;                     // m_PeakOn: kept and reported only
    int fspan = 0;                       // m_Span
    double ffs = 1.0;                    // the rate CFft::SetFFTParams got at the last Reset (:535)
    int fpos = 0, fcur = 0;              // m_FftBufPos and the carry buffer that holds those samples
    long long fcnt = -2;                 // m_DisplaySkipCounter while the receiver is in the FFT view

    int skip_now() const { return view == VIEW_FFT ? fft_skip_value(rate, sr) : skip_value(span, rate, sr); }
    void derive(int w) { skip = skip_now(); pix = pixel_time(span, w); }
    void on_display_rate(int r) { rate = r; skip = skip_now(); }                                // :247-258
    void on_horz_span(int s, int w)                                                             // :270-279
    {
        span = s;
        if (view == VIEW_TIME) { skip = skip_now(); pix = pixel_time(span, w); }
    }
    void reset(int w)                                                                           // :535-538, :541-548, :555-574
    {
        derive(w);
        ffs = sr; fspan = sr < kFftMaxRate ? fft_span(sr) : 0; fpos = 0; fcnt = -2;
        flags |= F_RESET;
    }
    void on_trigger_mode(int m, int w) { mode = m; reset(w); }                                  // :288-292
    void on_time_display(int timemode, int w) { view = timemode ? VIEW_TIME : VIEW_FFT; reset(w); }   // :282-286
    void on_enable_peak(int on) { peak_on = on; flags |= F_PEAK; }                              // :334-343
    void time_plot_done() { if (mode != TRIG_PSINGLE && mode != TRIG_NSINGLE) flags |= F_REARM; }   // :995-999
    // the settings of one put of n samples at rate fs; takes the pending flags with it
    void prepare(int n, double fs, int w, ChanParam &p, int h = 100, int cpx = 0)
    {
        p.n = n;
        if (n > 0 && sr != fs) { sr = fs; reset(w); p.n = 0; }      // :587-592: reset, and the call's samples are not used
        p.pix = pix; p.sr = sr; p.skip = skip; p.level = level; p.mode = mode; p.vert = vert;
        p.flags = flags;
        flags = 0;
        p.view = view; p.h = h;
        p.fill = fpos; p.cur = fcur; p.frames = p.first = p.count = 0; p.step = 1; p.pos_end = fpos; p.cnt_end = (int)fcnt;
        p.map = make_fft_map(fspan, cpx, ffs, w, h);
        if (view == VIEW_FFT && p.n > 0) {
            const FftPlan f = fft_plan(fpos, fcnt, skip, p.n);
            p.frames = (int)f.frames; p.count = (int)f.count;
            if (f.count > 0) { p.first = (int)f.first; p.step = (int)(f.count > 1 ? f.step : 1); }
            fpos = p.pos_end = f.pos_end; fcnt = f.cnt_end; p.cnt_end = (int)f.cnt_end;
            if (f.frames > 0) fcur ^= 1;                 // the new partial frame goes into the other carry buffer
        }
    }
};

}  // namespace sc
}  // namespace csdr
