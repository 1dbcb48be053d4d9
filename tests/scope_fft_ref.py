"""A line-for-line Python restatement of the FFT view of the reference's test bench (gui/testbench.cpp): the frequency
branch of DisplayData, complex :594-611 and real :654-672; Reset's FFT part :535-538, :550-557, :570-574; OnDisplayRate
:257; OnHorzSpan :272-273; OnTimeDisplay :282-286; OnEnablePeak :334-343; DrawFftPlot :1005-1068.  It subclasses
scope_ref.RefScope (the time view, which it leaves as it is) and wraps the fp64 oracle's CFft for SetFFTParams,
SetFFTAve(0), PutInDisplayFFT, GetScreenIntegerFFTData and m_pFFTAveBuf.  The deviations of include/cutesdr_mi.h are
restated too: a new object is in the time view, every used frame is drawn at once, a sample-rate change resets at
once, and OutBuf[w] is dropped (the oracle's wrapper returns w entries)."""
import numpy as np

import scope_ref as R

TEST_FFTSIZE = 2048
TOL_NEAR, TOL_MID, TOL_DEEP = 0.001, 0.05, 0.2            # assert_spectrum_close's three classes, in bels
FLOOR_BELS = -15.0                                        # ... which says nothing at or below this


def c_rem(a, b):
    """C's %: the sign of the dividend"""
    return a - b * R.c_div(a, b)


def spectrum_tol(want):
    """the tolerance assert_spectrum_close (tests/test_fft_resampler_gpu.py) gives each bin of `want` (bels)"""
    tol = np.full(want.shape, TOL_DEEP)
    tol[want > want.max() - 9.0] = TOL_MID
    tol[want > want.max() - 6.0] = TOL_NEAR
    return tol


class Draw:
    """one drawn frame: the oracle's bels, the mapping's arguments and y"""
    __slots__ = ("bels", "cpx", "start", "stop", "y", "fs")

    def __init__(self, bels, cpx, start, stop, y, fs):
        self.bels, self.cpx, self.start, self.stop, self.y, self.fs = bels, cpx, start, stop, y, fs


class RefFftScope(R.RefScope):
    """one CTestBench, both views; member names as the reference's"""

    def __init__(self, orc):
        self.orc = orc
        self.m_Fft = orc.CFft()
        self.m_Fft.SetFFTAve(0)                          # :132: an average size of 1 (dsp/fft.cpp:103-113)
        self.m_TimeDisplay = True                        # deviation: the constructor's default is False (:110)
        self.m_PeakOn = False                            # :107
        self.m_MaxdB, self.m_MindB = 10, 10 - 18 * 10    # :96-98, :1257 (DrawFreqOverlay, before anything is drawn)
        self.m_NewDataIsCpx = False
        self.m_FftInBuf = np.zeros(TEST_FFTSIZE, dtype=np.complex128)
        self.m_FftBufPos = 0
        self.m_FftPkBuf = [100] * R.TB_MAX_SCREENSIZE
        self.fft_screen = [0] * R.TB_MAX_SCREENSIZE      # the last drawn fftbuf
        self.fft_cpx = False                             # ... and how it was mapped
        self.fft_emits = 0                               # NewFftData
        self.total = 0                                   # CFft::m_TotalCount since the last Reset
        self.bels = np.zeros(TEST_FFTSIZE)               # m_pFFTAveBuf
        self.draws = []                                  # every Draw since the caller last cleared it
        self.track = True                                # keep the pixels' tolerance intervals (see pixel_interval)
        self.scr_lo = self.scr_hi = np.zeros(R.TB_MAX_SCREENSIZE, dtype=np.int64)
        super().__init__()                               # ends in Reset()

    # ------------------------------------------------------------------ slots
    def _skip(self):
        if self.m_TimeDisplay:
            super()._skip()
        else:                                            # :257, :570, into a qint32
            self.m_DisplaySkipValue = R.c_int(self.m_DisplaySampleRate / (TEST_FFTSIZE * self.m_DisplayRate))

    def OnHorzSpan(self, span):                          # :270-279
        if self.m_TimeDisplay:
            super().OnHorzSpan(span)
        else:
            self.m_HorzSpan = span

    def OnTimeDisplay(self, timemode):                   # :282-286
        self.m_TimeDisplay = bool(timemode)
        self.Reset()

    def OnEnablePeak(self, enablepeak):                  # :334-343
        for i in range(R.TB_MAX_SCREENSIZE):
            self.m_FftPkBuf[i] = self.h
            self.m_TimeBuf1[i] = 0
            self.m_TimeBuf2[i] = 0
        self.m_PeakOn = bool(enablepeak)
        self.pk_lo = np.full(R.TB_MAX_SCREENSIZE, self.h, dtype=np.int64)
        self.pk_hi = self.pk_lo.copy()

    def Reset(self):
        self.m_Fft.SetFFTParams(TEST_FFTSIZE, False, 0.0, self.m_DisplaySampleRate)    # :535
        self.fft_fs = self.m_DisplaySampleRate
        self.m_FftBufPos = 0                             # :536
        self.m_Span = R.c_int(self.m_DisplaySampleRate)  # :537, a qint32
        self.m_Span = self.m_Span - c_rem(self.m_Span + 5, 10) + 5                     # :538
        super().Reset()                                  # :541-548, the rings of :555-560, the skip value of the view, :574
        self.m_FftInBuf[:] = 0                           # :550-554
        for i in range(R.TB_MAX_SCREENSIZE):
            self.m_FftPkBuf[i] = self.h                  # :557
        self.m_Fft.ResetFFT()                            # :573
        self.total = 0
        self.bels = np.zeros(TEST_FFTSIZE)
        self.pk_lo = np.full(R.TB_MAX_SCREENSIZE, self.h, dtype=np.int64)      # the peak's interval: the running minimum
        self.pk_hi = self.pk_lo.copy()                                         # of the draws' lo and of their hi

    # ------------------------------------------------------------------ DisplayData
    def DisplayData(self, re, im, samplerate, on_emit=None):
        if self.m_TimeDisplay:
            return super().DisplayData(re, im, samplerate, on_emit)
        if self.m_DisplaySampleRate != samplerate:       # :587-592
            self.m_DisplaySampleRate = samplerate
            self.Reset()
            return
        self.m_NewDataIsCpx = im is not None             # :593, :653
        x = np.asarray(re, dtype=np.float64) + 1j * (np.asarray(im, dtype=np.float64) if im is not None else 0.0)
        i = 0
        while i < len(x):                                # :597-610, a frame's worth at a time
            k = min(TEST_FFTSIZE - self.m_FftBufPos, len(x) - i)
            self.m_FftInBuf[self.m_FftBufPos:self.m_FftBufPos + k] = x[i:i + k]
            self.m_FftBufPos += k
            i += k
            if self.m_FftBufPos >= TEST_FFTSIZE:
                self.m_FftBufPos = 0
                self.m_DisplaySkipCounter += 1
                if self.m_DisplaySkipCounter >= self.m_DisplaySkipValue:
                    self.m_DisplaySkipCounter = 0
                    self.total = self.m_Fft.PutInDisplayFFT(self.m_FftInBuf)
                    self.bels = self.m_Fft.ave_buf()
                    self.fft_emits += 1
                    self.emits += 1                      # get_emits counts NewFftData in this view
                    self.DrawFftPlot()                   # deviation: at once

    def map_args(self, cpx):
        start = R.c_div(-self.m_Span, 2) if cpx else 0   # :1031, :1040
        return start, R.c_div(self.m_Span, 2)

    def DrawFftPlot(self):                               # :1014-1052
        cpx = self.m_NewDataIsCpx
        start, stop = self.map_args(cpx)
        _, y = self.m_Fft.GetScreenIntegerFFTData(self.h, self.w, self.m_MaxdB, self.m_MindB, start, stop)
        y = [int(v) for v in y]
        for i in range(self.w):
            self.fft_screen[i] = y[i]
            if y[i] < self.m_FftPkBuf[i]:
                self.m_FftPkBuf[i] = y[i]
        self.fft_cpx = cpx
        d = Draw(self.bels.copy(), cpx, start, stop, y, self.fft_fs)
        self.draws.append(d)
        if self.track:
            lo, hi = pixel_interval(d, self.h, self.w)
            assert (lo <= np.array(y)).all() and (np.array(y) <= hi).all()
            self.scr_lo, self.scr_hi = lo, hi
            self.pk_lo[:self.w] = np.minimum(self.pk_lo[:self.w], lo)
            self.pk_hi[:self.w] = np.minimum(self.pk_hi[:self.w], hi)

    # ------------------------------------------------------------------ readers
    def fft_state(self):
        return [self.m_FftBufPos, self.m_DisplaySkipCounter, self.m_DisplaySkipValue, self.total]


def map_lines(bels, fs, h, w, start, stop, maxdb=10.0, mindb=-170.0):
    """The restatement's own mapping of an array of 2048 bels: dsp/fft.cpp:323-407, OutBuf[w] dropped.  The oracle's
    CFft has no setter for m_pFFTAveBuf, so bels +- tol cannot go through its GetScreenIntegerFFTData; these are its
    lines, and test_scope_fft_host.py pins them to the oracle on the oracle's own bels."""
    n = TEST_FFTSIZE
    off, gain = maxdb / 10.0, -10.0 / (maxdb - mindb)
    maxbin = n - 1
    bmin = min(max(R.c_int(float(start) * float(n) / fs) + n // 2, 0), maxbin)
    bmax = min(max(R.c_int(float(stop) * float(n) / fs) + n // 2, 0), maxbin)
    y = np.clip(np.trunc(float(h) * gain * (np.asarray(bels, dtype=np.float64) - off)).astype(np.int64), 0, h)   # :369-373
    out = [None] * (w + 1)
    if bmax - bmin > w:
        xprev, ymax = -1, 10000
        for i in range(bmin, bmax + 1):
            x = ((i - bmin) * w) // (bmax - bmin)
            if x == xprev:
                if y[i] < ymax:
                    out[x] = int(y[i]); ymax = int(y[i])
            else:
                out[x] = int(y[i]); xprev = x; ymax = int(y[i])
    else:
        for x in range(w):
            out[x] = int(y[bmin + (x * (bmax - bmin)) // w])
    assert all(v is not None for v in out[:w])           # every pixel below w receives a bin
    return out[:w]


def pixel_interval(d, h, w):
    """[lo, hi] per pixel of one Draw: the mapping on bels + tol and on bels - tol (it is monotone, falling)"""
    tol = spectrum_tol(d.bels)
    lo = map_lines(d.bels + tol, d.fs, h, w, d.start, d.stop)
    hi = map_lines(d.bels - tol, d.fs, h, w, d.start, d.stop)
    return np.array(lo), np.array(hi)


def assert_above_floor(draws):
    """the condition under which the bels' tolerance says something about every bin: on the oracle alone"""
    for d in draws:
        assert d.bels.min() > FLOOR_BELS, d.bels.min()


def feed_signal(c, n, fs, cpx, seed=4321):
    """row c: tones at -20 and -30.5 dBFS plus Gaussian noise at -40 dBFS on the 16-bit scale (feed_signal of the
    display-stream test with the noise raised), fp32; real rows are the real part of the same"""
    from util_signals import FULL_SCALE
    rng = np.random.default_rng(seed + c)
    t = np.arange(n, dtype=np.float64)
    amp, sig = FULL_SCALE * 0.1, FULL_SCALE * 10 ** (-40 / 20.0)
    f1 = 0.11 + 0.07 * (c % 5)
    x = amp * np.exp(2j * np.pi * f1 * t) + 0.3 * amp * np.exp(-2j * np.pi * 0.31 * t) \
        + sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64) if cpx else x.real.astype(np.float32)


class RefFftBatch(R.RefBatch):
    """restatements behind the batch's interface"""

    def __init__(self, orc, channels=8):
        self.r = [RefFftScope(orc) for _ in range(channels)]

    def OnTimeDisplay(self, v, channel=-1): self._each("OnTimeDisplay", (v,), channel)
    def OnEnablePeak(self, v, channel=-1): self._each("OnEnablePeak", (v,), channel)
