// display_plan.hpp -- the frame logic of the display path of CSdrInterface::ProcessIQData (reference
// interface/sdrinterface.cpp:889-907) as a pure host function: which of the frames that complete in one call reach
// PutInDisplayFFT, and the carry / skip counter / gate state after the call.  Every channel of a batch gets the same
// samples per call, so one plan serves them all -- or, in the row form, one plan per row over the shared frame position
// (display_rows_plan).  Host logic (capi_fft.hip, and capi_hosttest.hip for the CPU tests); SpecRow is what the kernels
// read of it.
#pragma once
#include <algorithm>

namespace csdr {

struct DisplayState {
    int pos = 0;          // P: samples of the partial frame carried into the next call (m_FftBufPos / 2)
    int skip = 0;         // m_DisplaySkipValue (0 and 1: every frame)
    int counter = 0;      // m_DisplaySkipCounter
    int gated = 0;        // the m_ScreenUpateFinished handshake is on
    int ready = 1;        // m_ScreenUpateFinished
};

struct DisplayPlan {
    long long start;      // first used frame's first sample, relative to the call's first sample (>= -P: negative = in the carry)
    long long step;       // samples between used frames (a multiple of N)
    int count;            // used frames: each one a PutInDisplayFFT + emit NewFftData()
    DisplayState next;    // the state after the call
};

// SetMaxDisplayRate (sdrinterface.h:112-114): m_DisplaySkipValue = m_SampleRate / (m_FftSize * m_MaxDisplayRate),
// the quotient of a double truncated by the assignment to qint32
inline int display_skip_value(double sample_rate, int fft_size, int max_display_rate)
{
    return (int)(sample_rate / (double)((long long)fft_size * max_display_rate));
}

// n samples of every row through the loop of sdrinterface.cpp:889-907 with frames of N samples
inline DisplayPlan display_plan(const DisplayState &s, long long n, int N)
{
    DisplayPlan p;
    p.next = s;
    const long long avail = (long long)s.pos + n;
    const long long frames = avail / N;                   // frames that complete in this call (m_FftBufPos >= m_FftSize*2)
    p.next.pos = (int)(avail - frames * N);
    // ++m_DisplaySkipCounter >= m_DisplaySkipValue: with a value of 0 or 1 every frame; otherwise the frames where the
    // counter reaches the value, the first of them after (value - 1 - counter) more frames
    const long long S = s.skip > 1 ? s.skip : 1;
    const long long first = s.counter < S ? S - 1 - s.counter : 0;
    long long used = frames > first ? (frames - 1 - first) / S + 1 : 0;
    if (used > 0) p.next.counter = (int)(frames - 1 - (first + (used - 1) * S));
    else p.next.counter = (int)(s.counter + frames);
    p.start = -(long long)s.pos + first * N;
    p.step = S * N;
    // the gate drops a selected frame without touching the counter, and a used frame closes it: one frame per call
    // at most, none until ScreenUpdateDone()
    if (s.gated && used > 0) {
        if (!s.ready) used = 0;
        else { used = 1; p.next.ready = 0; }
    }
    p.count = (int)used;
    return p;
}


// ---- the row form: skip value, counter, gate and ready per row, the frame position shared ----
// One entry of a launch's table of ACTIVE rows (a row that uses no frame is in no table): the kernels find their row
// through it instead of through the block index (spectrum_kernels.h, display_stream_kernels.h).
struct SpecRow {
    int row;              // the channel
    int nframes;          // frames of this row in this launch (>= 1)
    int ave_size;         // the row's m_AveSize
    int pad;
    long long start;      // first frame's first sample, relative to the call's first sample (negative: in the carry)
    long long step;       // samples between the row's frames
};

// how a row-form call is cut into launches, in stream order: first the gathered frames (read through the frame gather
// into the staging rows: the frame that begins in the carry, frames in front of first_loaded, and every frame where the
// size or the call has no stream loaders), then the frames the stream loaders read where they lie
struct DisplayRowsSplit {
    int ngath, nload;         // entries of the two tables
    int max_gath, max_load;   // the largest nframes of each
    int max_count;            // the largest per-row count: the call's return value
    int next_pos;             // the shared frame position after the call
};

// n samples of every row: rows[r] (its pos is ignored: `pos` is the one of the object) -> next[r], counts[r] used frames
// of row r, and the two tables (room for nrows entries each).  loaders: this size and call have stream loaders, which
// take frames whose first sample is >= first_loaded (>= 0).  sorted: tables by falling frame count, so that the rows with
// a frame of index k are the first entries (the multi-launch sizes walk frame by frame).
inline DisplayRowsSplit display_rows_plan(const DisplayState *rows, const int *ave, int nrows, int pos, long long n, int N,
                                          bool loaders, long long first_loaded, bool sorted, DisplayState *next,
                                          int *counts, SpecRow *gath, SpecRow *load)
{
    DisplayRowsSplit d{0, 0, 0, 0, 0, pos};
    for (int r = 0; r < nrows; r++) {
        DisplayState s = rows[r];
        s.pos = pos;
        const DisplayPlan p = display_plan(s, n, N);
        next[r] = p.next;
        d.next_pos = p.next.pos;
        counts[r] = p.count;
        if (p.count == 0) continue;
        if (p.count > d.max_count) d.max_count = p.count;
        int ng = p.count;
        if (loaders)
            for (ng = 0; ng < p.count && p.start + ng * p.step < first_loaded; ) ng++;
        if (ng > 0) {
            gath[d.ngath++] = SpecRow{r, ng, ave[r], 0, p.start, p.step};
            if (ng > d.max_gath) d.max_gath = ng;
        }
        if (p.count > ng) {
            load[d.nload++] = SpecRow{r, p.count - ng, ave[r], 0, p.start + ng * p.step, p.step};
            if (p.count - ng > d.max_load) d.max_load = p.count - ng;
        }
    }
    if (sorted) {
        auto longer = [](const SpecRow &x, const SpecRow &y) { return x.nframes != y.nframes ? x.nframes > y.nframes : x.row < y.row; };
        std::sort(gath, gath + d.ngath, longer);
        std::sort(load, load + d.nload, longer);
    }
    return d;
}

}  // namespace csdr
