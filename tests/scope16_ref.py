"""The int16 overloads of the reference's test bench, restated line for line on top of scope_ref.py (time view) and
scope_fft_ref.py (FFT view): DisplayData(int, TYPEMONO16*, ...) gui/testbench.cpp:702-754 and DisplayData(int,
TYPESTEREO16*, ...) :761-814 -- the only overloads PROFILE_5 (interface/soundout.cpp:207, :265) can reach.  The checker
of csdr_scope_batch_put_mono16 / _put_stereo16.

There is no compiled second checker for these lines: gui/testbench.cpp is a QDialog and needs Qt, so the reference's
own object code cannot be built into oracle/_ref/ the way its dsp/ files are.  The restatement is held against the
source by reading; everything below it (ChkForTrigger, the ring, the FFT branch's CFft) is the code the merged time-
and FFT-view tests already pin.

What differs from the TYPEREAL / TYPECPX overloads:
  stereo  time view: ChkForTrigger((int)pBuf[i].re), the ring gets re and im (:800-802); FFT view: (re, im),
          m_NewDataIsCpx = true (:771, :777-778) -- the complex overload on integers.
  mono    FFT view: m_FftInBuf gets (x, x), BOTH parts (:718-719), m_NewDataIsCpx = false (:712): the screen starts at
          0 Hz.  Time view: the ring gets pBuf[i] and 0 (:742-743), but ChkForTrigger -- and with it m_PreviousSample
          -- sees pBuf[i<<1] (:741).
Deviation (7) of include/cutesdr_mi.h: index 2i counts inside the call's n samples; for 2i >= n the trigger sample is 0
(the reference reads past its buffer there)."""
import numpy as np

import scope_fft_ref as F
import scope_ref as R


class Int16Overloads:
    """mixed into a RefScope: the two overloads beside DisplayData"""
    past = 0                                             # trigger reads with 2i >= n (deviation (7)), counted

    def DisplayStereo16(self, re, im, samplerate):       # :761-814: the complex overload's lines on integers
        return self.DisplayData([int(v) for v in re], [int(v) for v in im], samplerate)

    def DisplayMono16(self, buf, samplerate):            # :702-754
        if not getattr(self, "m_TimeDisplay", True):
            return self._mono_fft(buf, samplerate)
        if self.m_DisplaySampleRate != samplerate:       # :706-711
            self.m_DisplaySampleRate = samplerate
            self.Reset()
            return
        w, n = self.w, len(buf)
        for i in range(n):                               # :734-752
            intime = float(self.m_TimeInPos) / samplerate
            scrntime = float(self.m_TimeScrnPos) * self.m_TimeScrnPixel
            self.m_TimeInPos += 1
            while intime >= scrntime:
                if 2 * i < n:
                    t = int(buf[i << 1])                 # :741
                else:
                    t = 0                                # deviation (7)
                    self.past += 1
                self.ChkForTrigger(t)
                a = int(buf[i])
                self.log.append((a, 0))
                self.m_TimeBuf1[self.m_TimeScrnPos] = a  # :742-743
                self.m_TimeBuf2[self.m_TimeScrnPos] = 0
                self.m_TimeScrnPos += 1
                scrntime = float(self.m_TimeScrnPos) * self.m_TimeScrnPixel
                if self.m_TimeScrnPos >= w:
                    self.m_TimeScrnPos = 0
                    self.m_TimeInPos = 0
                    break


class RefScope16(Int16Overloads, R.RefScope):
    """the time view alone"""


class RefFftScope16(Int16Overloads, F.RefFftScope):
    """both views"""

    def _mono_fft(self, buf, samplerate):                # :706-731
        if self.m_DisplaySampleRate != samplerate:
            self.m_DisplaySampleRate = samplerate
            self.Reset()
            return
        self.m_NewDataIsCpx = False                      # :712
        x = np.asarray(buf, dtype=np.float64)
        x = x + 1j * x                                   # :718-719
        i = 0
        while i < len(x):                                # :716-730, a frame's worth at a time
            k = min(F.TEST_FFTSIZE - self.m_FftBufPos, len(x) - i)
            self.m_FftInBuf[self.m_FftBufPos:self.m_FftBufPos + k] = x[i:i + k]
            self.m_FftBufPos += k
            i += k
            if self.m_FftBufPos >= F.TEST_FFTSIZE:
                self.m_FftBufPos = 0
                self.m_DisplaySkipCounter += 1
                if self.m_DisplaySkipCounter >= self.m_DisplaySkipValue:
                    self.m_DisplaySkipCounter = 0
                    self.total = self.m_Fft.PutInDisplayFFT(self.m_FftInBuf)
                    self.bels = self.m_Fft.ave_buf()
                    self.fft_emits += 1
                    self.emits += 1
                    self.DrawFftPlot()                   # deviation (6): at once


def _put16(refs, rows, pos, n, rates):
    """rows: numpy int16 [channels, T] (mono) or [channels, T, 2] (stereo)"""
    for c, r in enumerate(refs):
        if n[c] == 0:
            continue
        x = rows[c, pos:pos + n[c]]
        if rows.ndim == 3:
            r.DisplayStereo16(x[:, 0].tolist(), x[:, 1].tolist(), rates[c])
        else:
            r.DisplayMono16(x.tolist(), rates[c])


class RefBatch16(R.RefBatch):
    def __init__(self, channels=16):
        self.r = [RefScope16() for _ in range(channels)]

    def put(self, rows, pos, n, rates):
        _put16(self.r, rows, pos, n, rates)


class RefFftBatch16(F.RefFftBatch):
    def __init__(self, orc, channels=8):
        self.r = [RefFftScope16(orc) for _ in range(channels)]

    def put(self, rows, pos, n, rates):
        _put16(self.r, rows, pos, n, rates)


def rows16(stereo, n=R.N_SAMPLES):
    """scope_ref's scenario rows cast to int16 (truncation, as (int) does): [16, n], or [16, n, 2] for stereo"""
    x = np.stack([R.signal(c, n, stereo) for c in range(16)])
    if not stereo:
        return np.trunc(x).astype(np.int16)
    return np.stack([np.trunc(x.real), np.trunc(x.imag)], axis=-1).astype(np.int16)


_TRACES = {}


def trace(k, stereo, events_key=None, events=None):
    """scope_ref.trace for the int16 rows: the restatement over the scenario, computed once"""
    key = (k, stereo, events_key)
    if key not in _TRACES:
        rows = rows16(stereo)
        ref = RefBatch16()
        R.configure(ref, k)
        calls = []
        R.run(ref, rows, k, R.cuts(), events,
              record=lambda i, emits: calls.append((emits, {c: ref.screen(c) for c, e in enumerate(emits) if e})))
        _TRACES[key] = (rows, calls, [ref.state(c) for c in range(16)], ref.totals(), [ref.screen(c) for c in range(16)],
                        sum(r.past for r in ref.r))
    return _TRACES[key]


def check(dut, k, stereo, events_key=None, events=None):
    """scope_ref.check for the int16 rows: dut (configured here) against the restatement -- the emits of every call, the
    screen of every receiver whenever it emitted, at the end every state and screen.  Returns (totals, trigger reads
    past n)."""
    rows, calls, states, totals, screens, past = trace(k, stereo, events_key, events)
    R.configure(dut, k)

    def record(i, emits):
        assert emits == calls[i][0], (i, emits, calls[i][0])
        for c, scr in calls[i][1].items():
            assert dut.screen(c) == scr, (i, c)

    R.run(dut, rows, k, R.cuts(), events, record=record)
    dut.put(rows, 0, [0] * 16, [r[1] for r in R.receivers(k)])                    # a put of nothing applies the last time_plot_done
    for c in range(16):
        assert dut.state(c) == states[c], (c, dut.state(c), states[c])
        assert dut.screen(c) == screens[c], c
    return totals, past
