// plotter_host.hpp -- the batch plotter's arithmetic that host and device share: one CPlotter's display state
// (reference gui/plotter.cpp: constructor :100-114, resizeEvent :374-389, draw :408-480, DrawOverlay's m_MindB :597;
// gui/plotter.h:32-44 for the setters) and the bels -> pixel mapping of CFft::GetScreenIntegerFFTData (dsp/fft.cpp:
// 308-410) as csdr_fft_batch_get_screen transcribes it (capi_fft.hip), turned round so that it is evaluated per PIXEL.
//
// Why a pixel can be evaluated alone.  In the "more bins than pixels" branch bin i goes to pixel x(i) = (i - bin_min) *
// w / range, range = bin_max - bin_min > w, which is monotone in i and steps by at most one: the bins of pixel x are the
// contiguous run k = i - bin_min with ceil(x range / w) <= k <= ceil((x + 1) range / w) - 1, never empty for x < w, and
// the pixel shows the smallest level of its run (:372-389; k = range would go to pixel w, which is dropped as
// csdr_fft_batch_get_screen drops it).  The level clamp((int)((double)H * gain * ((double)ave - off))) is monotone in
// ave -- non-increasing while gain < 0 (m_MaxdB > m_MindB), non-decreasing when a stale m_MindB lies above m_MaxdB -- so
// the smallest level of a run, at every height H, is the level of the run's largest ave (or, with gain > 0, of its
// smallest: run_keeps_smallest): one pass over the bels gives the waterfall line (H = 255) and the trace (H = the 2D
// height).  In the
// other branch pixel x reads the one bin bin_min + (min(x, n - 1) * range) / w (:391-407 with the n-entry translate
// table).  With the invert flag bin i is read at n - i, clamped to n - 1 (the reference reads one past the end there):
// the run of a pixel stays contiguous in memory, only reversed.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>

namespace csdr {
namespace pl {

constexpr int kMaxW = 4096;                              // MAX_SCREENSIZE (gui/plotter.cpp:48)
constexpr int kVertDivs = 14;                            // VERT_DIVS (gui/plotter.h:16)
constexpr int kOverloadLimit = 10;                       // OVERLOAD_DISPLAY_LIMIT (gui/plotter.cpp:50)
constexpr unsigned kBlack = 0xff000000u;                 // Qt::black as the waterfall's 0xFFRRGGBB

// (int) of a double, saturating where C leaves the conversion undefined
__host__ __device__ inline int sat_int(double x)
{
    if (!(x == x)) return 0;
    if (x >= 2147483647.0) return INT_MAX;
    if (x <= -2147483648.0) return INT_MIN;
    return (int)x;
}

// m_BinMin, m_BinMax and the branch of a view (fft.cpp:333-349)
struct Map {
    int bin_min, bin_max;
    int bins;                                            // 1: more bins than pixels
};
__host__ __device__ inline Map make_map(int n, double fs, int span, int w)
{
    const int start = -span / 2, stop = span / 2, maxbin = n - 1;      // draw()'s -m_Span/2, m_Span/2 on a qint32
    Map m;
    m.bin_min = sat_int((double)start * (double)n / fs);
    m.bin_max = sat_int((double)stop * (double)n / fs);
    m.bin_min = m.bin_min > INT_MAX - n ? INT_MAX : m.bin_min + n / 2;
    m.bin_max = m.bin_max > INT_MAX - n ? INT_MAX : m.bin_max + n / 2;
    if (m.bin_min < 0) m.bin_min = 0;
    if (m.bin_min >= maxbin) m.bin_min = maxbin;
    if (m.bin_max < 0) m.bin_max = 0;
    if (m.bin_max >= maxbin) m.bin_max = maxbin;
    m.bins = (m.bin_max - m.bin_min) > w;
    return m;
}

// where bin i of the display-order average lies (capi_fft.hip:443-444)
__host__ __device__ inline int bin_index(int n, int invert, int i)
{
    const int b = invert ? n - i : i;
    return b >= n ? n - 1 : b;
}

// the entries ave[lo..hi] (inclusive, lo <= hi, both within [0, n)) that pixel x < w shows; n <= 65536 and w <= 4096
// keep every product below 2^31
__host__ __device__ inline void pixel_bins(const Map &m, int n, int invert, int w, int x, int *lo, int *hi)
{
    const int range = m.bin_max - m.bin_min;
    int i0, i1;
    if (m.bins) {
        i0 = m.bin_min + (x * range + w - 1) / w;
        i1 = m.bin_min + ((x + 1) * range + w - 1) / w - 1;
    } else {
        const int xi = x < n ? x : n - 1;                // the translate table has n entries
        i0 = i1 = m.bin_min + (xi * range) / w;
    }
    const int a = bin_index(n, invert, i0), b = bin_index(n, invert, i1);
    *lo = a < b ? a : b; *hi = a < b ? b : a;
}

// gain and offset of a dB range (fft.cpp:318-319)
__host__ __device__ inline double db_gain(int max_db, int min_db) { return -10.0 / ((double)max_db - (double)min_db); }
__host__ __device__ inline double db_off(int max_db) { return (double)max_db / 10.0; }

// the level of one bel at height h, in the operation order of capi_fft.hip:445-447
__host__ __device__ inline int level(int h, double gain, double off, float ave)
{
    const double t = (double)h * gain * ((double)ave - off);
    if (!(t > 0.0)) return 0;
    return t >= (double)h ? h : (int)t;
}

// Which bel of a run gives the run's smallest level.  m_MindB is stale until UpdateOverlay (and for ever in a view
// without a 2D pixmap), so m_MaxdB < m_MindB can happen: then gain > 0, the level RISES with the bel, and the smallest
// level of a run is the level of its smallest bel.  (m_MaxdB == m_MindB: gain is -infinity and level() steps from h
// to 0 at ave == off, still non-increasing.)
__host__ __device__ inline int run_keeps_smallest(int max_db, int min_db) { return max_db < min_db; }
__host__ __device__ inline float run_keep(float kept, float v, int smallest)
{
    return smallest ? (v < kept ? v : kept) : (v > kept ? v : kept);
}
__host__ __device__ inline float run_start(int smallest) { return smallest ? __builtin_inff() : -__builtin_inff(); }

// the pen of draw() (:458-468): red while m_ADOverLoad or the FFT's overload flag holds; the one-shot counter lets a
// SetADOverload(true) stand for OVERLOAD_DISPLAY_LIMIT + 2 draws
__host__ __device__ inline int pen_step(int *ad_overload, int *counter, int fft_overload)
{
    if (!*ad_overload && !fft_overload) return 0;
    if ((*counter)++ > kOverloadLimit) { *counter = 0; *ad_overload = 0; }
    return 1;
}

// lanes that share a pixel in the draw kernel: the power of two at or above the bins of a pixel, 64 at the most
__host__ __device__ inline int group_lanes(const Map &m, int w)
{
    if (!m.bins || w < 1) return 1;
    const int per = (m.bin_max - m.bin_min + w - 1) / w;
    int g = 1;
    while (g < per && g < 64) g *= 2;
    return g;
}

// One CPlotter's settings as the host keeps them.  The ring of waterfall lines: `head` is the ring row of the newest
// line, image row r (newest first) is ring row (head + r) % wf_h, and only the first `filled` image rows have been
// drawn since the last resize -- the rest is black, whatever the memory holds.
struct View {
    int span = 50000, max_db = 0, min_db = -130, step = 10, percent = 50, running = 0;      // :100-114
    int width = 0, height = 0;                           // the widget's size
    int w = 0, h2d = 0, wf_h = 0;                        // the pixmaps' (:381-385)
    int row = 0;                                         // the spectrum row the view plots
    int head = 0, filled = 0, traced = 0;                // traced: the trace buffer holds a draw at this size
    int ad_cmd = -1;                                     // SetADOverload waiting for the next draw: -1 none, 0 / 1

    void update_overlay()                                // DrawOverlay (:597), which returns early on a null pixmap
    {
        if (w > 0 && h2d > 0) {
            const long long v = (long long)max_db - (long long)kVertDivs * step;
            min_db = v < INT_MIN ? INT_MIN : (v > INT_MAX ? INT_MAX : (int)v);
        }
    }
    void resize(int W, int H, bool forget_size = false)  // resizeEvent (:374-389)
    {
        if (forget_size || W != width || H != height) traced = 0;      // m_Size != size(): a new, black m_2DPixmap (:378-384)
        width = W; height = H;
        w = W; h2d = percent * H / 100; wf_h = (100 - percent) * H / 100;
        head = 0; filled = 0;                            // m_WaterfallPixmap.fill(Qt::black), on every event
        update_overlay();
    }
    void set_percent(int p) { percent = p; resize(width, height, true); }   // SetPercent2DScreen (plotter.h:35): m_Size = QSize(0,0) first
    void scroll()                                        // :425, and the new line becomes image row 0
    {
        if (wf_h < 1 || w < 1) return;
        head = (head + wf_h - 1) % wf_h;
        if (filled < wf_h) filled++;
    }
};

}  // namespace pl
}  // namespace csdr
