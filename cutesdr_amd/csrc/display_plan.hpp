// display_plan.hpp -- the frame logic of the display path of CSdrInterface::ProcessIQData (reference
// interface/sdrinterface.cpp:889-907) as a pure host function: which of the frames that complete in one call reach
// PutInDisplayFFT, and the carry / skip counter / gate state after the call.  Every channel of a batch gets the same
// samples per call, so one plan serves them all.  Host only (capi_fft.hip, and capi_hosttest.hip for the CPU tests).
#pragma once

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

}  // namespace csdr
