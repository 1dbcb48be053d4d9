"""Restatement of the reference's test-bench generator (gui/testbench.cpp: CreateGeneratorSamples :352-447 complex,
:454-517 real; the On... slots :225-244, :307-332; the generator part of Reset() :527-532, :575) in fp64, written from
the reference's text, and of the counter-based noise source from the comment in include/cutesdr_mi.h.  Nothing here
calls the library.

RefTestBench.create() has two forms that give the same bits: `literal=True` walks the samples one by one in Python
floats, exactly as the reference's loops read; the default does the same sequential fp64 additions with
numpy.add.accumulate (strictly left to right, so every partial sum is the loop's) and is fast enough for 2^21 samples.
test_testgen_host.py checks the two against each other.
"""
import math

import numpy as np

K_2PI = 2.0 * math.pi
MAX_AMPLITUDE = 32767.0
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
ATTEMPTS = 32


# ---------------------------------------------------------------------------------------------- noise source
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, c):
    return mix((seed + GOLDEN * (c + 1)) & M64)


def draws(seed, c, i, a):
    """the two 31-bit integers of attempt a of sample i of receiver c"""
    h = mix((key(seed, c) + GOLDEN * (32 * i + a)) & M64)
    return h >> 33, (h >> 2) & 0x7FFFFFFF


def _mix_np(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def gauss(seed, c, i0, n):
    """(g1, g2, attempts): the polar method's two terms u1*rad, u2*rad of samples i0..i0+n-1 (0 where all 32 attempts
    were rejected), and the attempt that was taken"""
    k = np.uint64(key(seed, c))
    i = np.uint64(i0) + np.arange(n, dtype=np.uint64)
    g1, g2 = np.zeros(n), np.zeros(n)
    att = np.full(n, -1)
    todo = np.arange(n)
    with np.errstate(over="ignore"):
        for a in range(ATTEMPTS):
            if todo.size == 0:
                break
            h = _mix_np(k + np.uint64(GOLDEN) * (np.uint64(32) * i[todo] + np.uint64(a)))
            k1 = (h >> np.uint64(33)).astype(np.float64)
            k2 = ((h >> np.uint64(2)) & np.uint64(0x7FFFFFFF)).astype(np.float64)
            u1 = 1.0 - 2.0 * k1 / 2147483647.0
            u2 = 1.0 - 2.0 * k2 / 2147483647.0
            r = u1 * u1 + u2 * u2
            ok = ~((r >= 1.0) | (r == 0.0))
            rad = np.sqrt(-2.0 * np.log(r[ok]) / r[ok])
            g1[todo[ok]] = u1[ok] * rad
            g2[todo[ok]] = u2[ok] * rad
            att[todo[ok]] = a
            todo = todo[~ok]
    return g1, g2, att


# ---------------------------------------------------------------------------------------------- the generator
class RefTestBench:
    """One CTestBench generator; members named after the reference's.  Units of the setters as the library's (Hz, Hz/s,
    seconds, dB); the reference's integer kHz / ms arguments are scaled by the caller."""

    def __init__(self, seed=0, channel=0):
        self.m_GenOn = False
        self.m_GenSampleRate = 1.0
        self.m_PulseWidth = .01
        self.m_PulsePeriod = .5
        self.m_PulseTimer = 0.0
        self.m_SweepStartFrequency = 0.0
        self.m_SweepStopFrequency = 0.0
        self.m_SweepRate = 0.0
        self.m_SignalPower = 0.0
        self.m_NoisePower = -160.0
        self.seed, self.channel, self.count = seed, channel, 0
        self.Reset()

    def OnSweepStart(self, hz):
        self.m_SweepStartFrequency = float(hz)
        self.m_SweepFrequency = self.m_SweepStartFrequency
        self.m_SweepAcc = 0.0

    def OnSweepStop(self, hz):
        self.m_SweepStopFrequency = float(hz)
        self.m_SweepFrequency = self.m_SweepStartFrequency
        self.m_SweepAcc = 0.0

    def OnSweepRate(self, rate):
        self.m_SweepRate = float(rate)
        self.m_SweepAcc = 0.0
        self.m_SweepRateInc = self.m_SweepRate / self.m_GenSampleRate

    def OnGenOn(self, on):
        self.m_GenOn = bool(on)

    def OnPulseWidth(self, s):
        self.m_PulseWidth = float(s)

    def OnPulsePeriod(self, s):
        self.m_PulsePeriod = float(s)

    def OnSignalPwr(self, db):
        self.m_SignalPower = float(db)
        self.m_SignalAmplitude = MAX_AMPLITUDE * math.pow(10.0, self.m_SignalPower / 20.0)

    def OnNoisePwr(self, db):
        self.m_NoisePower = float(db)
        self.m_NoiseAmplitude = MAX_AMPLITUDE * math.pow(10.0, self.m_NoisePower / 20.0)

    def SetSeed(self, seed):
        self.seed, self.count = seed, 0

    def Reset(self):
        self.m_SweepFrequency = self.m_SweepStartFrequency
        self.m_SweepFreqNorm = K_2PI / self.m_GenSampleRate
        self.m_SweepAcc = 0.0
        self.m_SweepRateInc = self.m_SweepRate / self.m_GenSampleRate
        self.m_SignalAmplitude = MAX_AMPLITUDE * math.pow(10.0, self.m_SignalPower / 20.0)
        self.m_NoiseAmplitude = MAX_AMPLITUDE * math.pow(10.0, self.m_NoisePower / 20.0)
        self.m_PulseTimer = 0.0

    def create(self, length, samplerate, real=False, literal=False, trace=None):
        """CreateGeneratorSamples: `length` samples (complex128, or float64 for the real overload), None when the
        generator is off.  A changed sample rate resets before the first sample (the library's documented choice).
        trace: optional dict that receives the per-sample frequency, phase before the sample and gate."""
        if not self.m_GenOn:
            return None
        if self.m_GenSampleRate != samplerate:
            self.m_GenSampleRate = float(samplerate)
            self.Reset()
        noisy = self.m_NoisePower > -160.0
        g1 = g2 = None
        if noisy:
            g1, g2, _ = gauss(self.seed, self.channel, self.count, length)
        self.count += length
        f = self._literal if literal else self._fast
        amp, acc, freq = f(length)
        if trace is not None:
            trace["freq"], trace["acc"], trace["gate"] = freq, acc, amp != 0.0
        if real:
            out = 3.0 * amp * np.cos(acc)
            if noisy:
                out = out + self.m_NoiseAmplitude * g1
            return out
        re, im = amp * np.cos(acc), amp * np.sin(acc)
        if noisy:
            re = re + self.m_NoiseAmplitude * g1
            im = im + self.m_NoiseAmplitude * g2
        return re + 1j * im

    # the loop of :396-445 without the noise: per-sample amplitude, phase and frequency; state advanced, fmod at the end
    def _literal(self, length):
        amp, acc, freq = np.empty(length), np.empty(length), np.empty(length)
        for i in range(length):
            a = self.m_SignalAmplitude
            if self.m_PulseWidth > 0.0:
                self.m_PulseTimer += (1.0 / self.m_GenSampleRate)
                if self.m_PulseTimer > self.m_PulsePeriod:
                    self.m_PulseTimer = 0.0
                if self.m_PulseTimer > self.m_PulseWidth:
                    a = 0.0
            amp[i], acc[i], freq[i] = a, self.m_SweepAcc, self.m_SweepFrequency
            self.m_SweepAcc += (self.m_SweepFrequency * self.m_SweepFreqNorm)
            self.m_SweepFrequency += self.m_SweepRateInc
            if self.m_SweepFrequency >= self.m_SweepStopFrequency:
                self.m_SweepRateInc = 0.0
        self.m_SweepAcc = math.fmod(self.m_SweepAcc, K_2PI)
        return amp, acc, freq

    def _fast(self, length):
        n = length
        # pulse timer: sequential sums of 1/Fs from the current value, restarted from 0.0 after the first sum > period
        amp = np.full(n, self.m_SignalAmplitude)
        if self.m_PulseWidth > 0.0:
            d = 1.0 / self.m_GenSampleRate
            t = np.empty(n)
            pos = 0
            while pos < n:
                s = np.add.accumulate(np.concatenate(([self.m_PulseTimer], np.full(n - pos, d))))[1:]
                over = np.nonzero(s > self.m_PulsePeriod)[0]
                if over.size:
                    k = int(over[0])
                    t[pos:pos + k] = s[:k]
                    t[pos + k] = 0.0
                    self.m_PulseTimer = 0.0
                    pos += k + 1
                else:
                    t[pos:] = s
                    self.m_PulseTimer = float(s[-1])
                    pos = n
            amp[t > self.m_PulseWidth] = 0.0
        # frequency: sequential sums of the increment until the first value >= stop, constant after it
        freq = np.empty(n + 1)
        pos = 0
        freq[0] = self.m_SweepFrequency
        while pos < n:
            if self.m_SweepRateInc == 0.0:
                freq[pos + 1:] = freq[pos]
                break
            s = np.add.accumulate(np.concatenate(([freq[pos]], np.full(n - pos, self.m_SweepRateInc))))[1:]
            hit = np.nonzero(s >= self.m_SweepStopFrequency)[0]
            if hit.size:
                k = int(hit[0])
                freq[pos + 1:pos + k + 2] = s[:k + 1]
                self.m_SweepRateInc = 0.0
                pos += k + 1
            else:
                freq[pos + 1:] = s
                pos = n
        self.m_SweepFrequency = float(freq[n])
        acc = np.add.accumulate(np.concatenate(([self.m_SweepAcc], freq[:n] * self.m_SweepFreqNorm)))
        self.m_SweepAcc = math.fmod(float(acc[n]), K_2PI)
        return amp, acc[:n], freq[:n]


def literal_crossing(x0, d, limit, strict, cap=1 << 26):
    """first index i >= 1 with x_i > limit (strict) or >= limit of x_i = fl(x_{i-1} + d), and x_i; (None, x) if none
    within cap additions.  The plain sequential sums, in blocks."""
    x, i = float(x0), 0
    while i < cap:
        m = min(1 << 20, cap - i)
        s = np.add.accumulate(np.concatenate(([x], np.full(m, float(d)))))[1:]
        hit = np.nonzero(s > limit if strict else s >= limit)[0]
        if hit.size:
            return i + int(hit[0]) + 1, float(s[hit[0]])
        x, i = float(s[-1]), i + m
    return None, x


# ---------------------------------------------------------------------------------------------- shared test set-up
# The 16 receivers of the GPU parity and cut-invariance tests; the CPU tests check the tolerance's premise on the same
# frequencies.  (start Hz, stop Hz, rate Hz/s, width s, period s, signal dB, on)
FS1, FS2 = 2.0e6, 615384.6
RECEIVERS = [
    (100000.0, 100000.0, 0.0, 0.0, 0.5, 0.0, True),            # 0 constant tone, full scale
    (737123.5, 737123.5, 0.0, 0.0, 0.5, 0.0, True),            # 1 constant tone near Fs/2
    (-300000.0, 123456.0, 3.3e6, 0.0, 0.5, 0.0, True),         # 2 the sweep whose fp64 end is one sample late
    (-50000.0, 50000.0, 4.0e6, 0.0, 0.5, 0.0, True),           # 3 through zero, ends inside the stream
    (-400000.0, 900000.0, 1.0e6, 0.0, 0.5, -3.0, True),        # 4 through zero, still sweeping at the rate change
    (250000.0, 250000.0, 0.0, 0.001, 0.1, 0.0, True),          # 5 pulse 1 ms / 100 ms
    (-123456.789, -123456.789, 0.0, 0.01, 0.5, -6.0, True),    # 6 the constructor's pulse
    (200000.0, 100000.0, 1.0e6, 0.0, 0.5, 0.0, True),          # 7 start >= stop: one step, then constant
    (10000.0, 10000.0, 0.0, 0.0, 0.5, -160.0, True),           # 8 amplitude 3.3e-4 counts
    (55555.0, 66666.0, 1000.0, 0.001, 0.1, 0.0, False),        # 9 OFF: its row must stay as it was
    (-250000.0, -250000.0, 0.0, 0.2, 0.1, 0.0, True),          # 10 width >= period: timer runs, gate never closes
    (-500000.0, -100000.0, 2.0e6, 0.005, 0.02, -6.0, True),    # 11 pulsed sweep ending after 0.2 s
    (1000.0, 300000.0, 5.0e5, 0.0, 0.5, 0.0, True),            # 12 slots between calls (sweep start / stop)
    (0.0, 20000.0, 1.0e6, 0.0, 0.5, 0.0, True),                # 13 finished sweep re-armed by the rate slot
    (31250.0, 31250.0, 0.0, 0.003, 0.05, 0.0, True),           # 14 power, pulse and reset slots
    (1.0, 1.0, 0.0, 0.0, 0.5, -20.0, True),                    # 15 1 Hz; switched off for one call
]
CUTS = [2, 1 << 20, 6, 1022, 65534, 262146, 131070, 524290, 64506]           # 2^21 samples: odd multiples of 2, 2, 2^20
RATES = [FS1] * 6 + [FS2] * 3                                                 # the rate changes in mid-stream
# slots called before call k: (receiver, slot, value)
EVENTS = {
    2: [(12, "OnSweepStart", -100000.0), (13, "OnSweepRate", 2.0e6), (14, "OnSignalPwr", -10.0), (5, "OnNoisePwr", -160.0)],
    4: [(14, "OnPulseWidth", 0.002), (14, "OnPulsePeriod", 0.02), (12, "OnSweepStop", 50000.0), (13, "OnSweepStart", 5000.0)],
    5: [(14, "Reset", None), (6, "OnSignalPwr", 0.0), (11, "OnSweepRate", 3.0e6)],
    7: [(15, "OnGenOn", False), (3, "OnSweepRate", -1.0e6)],
    8: [(15, "OnGenOn", True), (10, "OnPulseWidth", 0.0)],
}
assert sum(CUTS) == 1 << 21 and len(RATES) == len(CUTS)


def slot(g, name, value, channel=None):
    """one slot of a RefTestBench (channel None) or of a TestGenBatch receiver"""
    args = () if value is None else (value,)
    if channel is None:
        getattr(g, name)(*args)
    else:
        getattr(g, name)(*args, channel=channel)


def configure(g, spec, channel=None, noise_db=None):
    start, stop, rate, width, period, sig, on = spec
    for name, v in (("OnSweepStart", start), ("OnSweepStop", stop), ("OnSweepRate", rate), ("OnPulseWidth", width),
                    ("OnPulsePeriod", period), ("OnSignalPwr", sig), ("OnGenOn", on)):
        slot(g, name, v, channel)
    if noise_db is not None:
        slot(g, "OnNoisePwr", noise_db, channel)


def ref_stream(c, real=False, noise_db=None, seed=0, call=256, cuts=CUTS, rates=RATES, events=EVENTS):
    """receiver c of the set-up above through the restatement, in `call`-sample calls between the events: the samples
    (NaN where the generator was off) as complex128 / float64"""
    r = RefTestBench(seed=seed, channel=c)
    configure(r, RECEIVERS[c], noise_db=noise_db)
    out = []
    for k, n in enumerate(cuts):
        for rc, name, v in events.get(k, ()):
            if rc == c:
                slot(r, name, v)
        for p in range(0, n, call):
            m = min(call, n - p)
            y = r.create(m, rates[k], real=real)
            out.append(np.full(m, np.nan, dtype=np.float64 if real else np.complex128) if y is None else y)
    return np.concatenate(out)


# ---------------------------------------------------------------------------------------------- noise tests
NOISE_SEEDS = (1, 2024)          # the seeds of the GPU noise test
NOISE_N = 1 << 20


def moments_ok(x, y, sigma):
    """the conditions of the noise tests: |mean| <= 6 sigma / sqrt(n) per component, |var / sigma^2 - 1| <= 6 sqrt(2/n),
    |corr(I, Q)| <= 6 / sqrt(n), |lag-1 autocorrelation| <= 6 / sqrt(n)"""
    n = len(x)
    out = {}
    for name, v in (("I", x), ("Q", y)):
        out["mean " + name] = (abs(v.mean()), 6.0 * sigma / math.sqrt(n))
        out["var " + name] = (abs(v.var() / sigma ** 2 - 1.0), 6.0 * math.sqrt(2.0 / n))
        z = v - v.mean()
        out["lag1 " + name] = (abs(np.dot(z[1:], z[:-1]) / np.dot(z, z)), 6.0 / math.sqrt(n))
    out["corr IQ"] = (abs(np.corrcoef(x, y)[0, 1]), 6.0 / math.sqrt(n))
    return out
