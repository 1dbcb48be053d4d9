"""A line-for-line fp64 restatement of the reference's noise blanker WITH its test-bench trace (dsp/noiseproc.cpp:
SetupBlanker :77-119, ProcessBlanker :121-176, m_TestBenchDataBuf :159, :163, :169).  Python floats are fp64, so every
line rounds as the reference's does.  It is the checker of csdr_noiseproc_batch_trace_last (PROFILE_7) and is pinned
to the reference's compiled code in tests/test_nbtrace_host.py: oracle.ref.CNoiseProc fed one sample per call hands
m_TestBenchDataBuf[0].re of every sample to the recording test bench, and the call's output pins the delayed sample."""
import numpy as np

MAX_WIDTH, MAX_DELAY, MAX_AVE, MAGAVE_TIME = 4096, 4096, 32768, 0.005      # :49-53


class RefNoiseProc:
    """one CNoiseProc; member names as the reference's"""

    def __init__(self):
        self.m_DelayBuf = [(0.0, 0.0)] * MAX_DELAY
        self.m_MagBuf = [0.0] * MAX_AVE
        self.m_On = self.m_Threshold = self.m_Width = None
        self.SetupBlanker(False, 50.0, 2.0, 1000.0)      # :64

    def SetupBlanker(self, On, Threshold, Width, SampleRate):
        if Threshold == self.m_Threshold and Width == self.m_Width and self.m_On == On and SampleRate == SampleRate:   # :79-85
            return
        self.m_On, self.m_Threshold, self.m_Width, self.m_SampleRate = On, Threshold, Width, SampleRate
        self.m_WidthSamples = int(Width * 1e-6 * SampleRate)                 # :92-96 (an int member)
        if self.m_WidthSamples < 1:
            self.m_WidthSamples = 1
        elif self.m_WidthSamples > MAX_WIDTH:
            self.m_WidthSamples = MAX_WIDTH
        self.m_MagSamples = int(MAGAVE_TIME * SampleRate)                    # :98
        assert self.m_MagSamples <= MAX_AVE - 1
        self.m_Ratio = .005 * Threshold * float(self.m_MagSamples)           # :100
        self.m_DelaySamples = self.m_WidthSamples // 2                       # :102
        self.m_Dptr = self.m_Mptr = self.m_BlankCounter = 0                  # :106-108
        self.m_MagAveSum = 0.0
        self.m_DelayBuf = [(0.0, 0.0)] * MAX_DELAY
        self.m_MagBuf = [0.0] * MAX_AVE

    def ProcessBlanker(self, x):
        """x: complex samples.  Returns (pOutData, m_TestBenchDataBuf, blanked) as complex128, complex128 and bool arrays
        (the reference's trace buffer has 4096 entries; here it is as long as the call).  A threshold of 0 divides by
        m_Ratio = 0: IEEE's inf / NaN, as the compiled code gives."""
        x = np.asarray(x, dtype=np.complex128)
        n = len(x)
        out, tb, blanked = np.zeros(n, dtype=np.complex128), np.zeros(n, dtype=np.complex128), np.zeros(n, dtype=bool)
        if not self.m_On:                                # :125-129: the trace shows pOutData, the data untouched
            return x.copy(), x.copy(), blanked
        re, im = x.real.tolist(), x.imag.tolist()
        ratio = self.m_Ratio
        for i in range(n):                               # :132-172
            mre, mim = abs(re[i]), abs(im[i])
            mag = mre if mre > mim else mim              # :137-139
            self.m_MagAveSum -= self.m_MagBuf[self.m_Mptr]                   # :143
            self.m_MagAveSum += mag                      # :144
            self.m_MagBuf[self.m_Mptr] = mag             # :145
            self.m_Mptr += 1
            if self.m_Mptr > self.m_MagSamples:
                self.m_Mptr = 0
            oldest = self.m_DelayBuf[self.m_Dptr]        # :150-153
            self.m_DelayBuf[self.m_Dptr] = (re[i], im[i])
            self.m_Dptr += 1
            if self.m_Dptr > self.m_DelaySamples:
                self.m_Dptr = 0
            if mag * ratio > self.m_MagAveSum:           # :155-158
                self.m_BlankCounter = self.m_WidthSamples
            tim = oldest[0] + oldest[1]                  # :159
            if self.m_BlankCounter:                      # :160-166
                self.m_BlankCounter -= 1
                tb[i] = complex(0.0, tim)
                blanked[i] = True
            else:                                        # :167-171
                s = self.m_MagAveSum
                tre = s / ratio if ratio != 0.0 else (float("nan") if s == 0.0 or s != s else float("inf") if s > 0 else float("-inf"))
                tb[i] = complex(tre, tim)
                out[i] = complex(oldest[0], oldest[1])
        return out, tb, blanked


def trace_fp32(tb):
    """m_TestBenchDataBuf rounded once to fp32, as complex64: what the device writes"""
    return np.asarray(tb, dtype=np.complex128).astype(np.complex64)


def datagram_like(n, seed, base=200, impulses=()):
    """Samples as datagrams decode to: integers of +-base (every fp64 sum of at most 32768 of them is exact in any
    order), with impulses [(index, re, im)] up to +-32767 put on top"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-base, base + 1, n).astype(np.float64) + 1j * rng.integers(-base, base + 1, n).astype(np.float64)
    for i, a, b in impulses:
        if i < n:
            x[i] = complex(a, b)
    return x
