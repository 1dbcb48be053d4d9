"""A line-for-line Python restatement of the time view of the reference's test bench (gui/testbench.cpp): Reset
:541-548, :555-565, :574; the slots :247-299; DisplayData's time branch, complex :583-636 and real :643-695;
ChkForTrigger :819-898; DrawTimePlot's vertical mapping and re-arm :973-999.  Python floats are fp64 and Python ints
are exact.  It is the checker of the batch scope (csdr_scope_batch) and is driven with exactly the calls the device
gets; the documented deviations of include/cutesdr_mi.h are restated too: (int) saturates and gives 0 for a NaN, a
sample-rate change resets at once, and DrawTimePlot's re-arm is the explicit call time_plot_done."""
import math

TB_MAX_SCREENSIZE = 2048
TRIG_OFF, TRIG_PNORM, TRIG_PSINGLE, TRIG_NNORM, TRIG_NSINGLE = range(5)
TRIGSTATE_WAIT, TRIGSTATE_CAPTURE, TRIGSTATE_DISPLAY, TRIGSTATE_WAITDISPLAY = range(4)
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31

# (w, span ms, sample rate): the configurations of the issue
CONFIGS = [(64, 10, 48000.0), (100, 3, 8000.0), (37, 1, 250000.0), (2048, 100, 12500.0), (33, 7, 7812.5), (1000, 100, 615384.6)]


def c_int(x):
    """(int)x of a float or double: truncation, saturating, NaN -> 0"""
    x = float(x)
    if x != x:
        return 0
    if x >= 2147483647.0:
        return INT_MAX
    if x <= -2147483648.0:
        return INT_MIN
    return int(x)


def c_div(a, b):
    """C's integer division: truncation towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class RefScope:
    """one CTestBench with m_TimeDisplay on; member names as the reference's"""

    def __init__(self):
        self.w, self.h = 100, 100                        # m_Rect, :94
        self.m_DisplaySampleRate = 1.0                   # :102
        self.m_DisplayRate = 10                          # :111-117
        self.m_HorzSpan = 100
        self.m_VertRange = 65000
        self.m_TrigLevel = 100
        self.m_TrigBufPos = 0
        self.m_TrigCounter = 0
        self.m_TrigState = TRIGSTATE_WAIT
        self.m_TrigIndex = TRIG_OFF
        self.m_TimeBuf1 = [0] * TB_MAX_SCREENSIZE
        self.m_TimeBuf2 = [0] * TB_MAX_SCREENSIZE
        self.m_TimeScrnBuf1 = [0] * TB_MAX_SCREENSIZE
        self.m_TimeScrnBuf2 = [0] * TB_MAX_SCREENSIZE
        self.emits = 0                                   # NewTimeData
        self.log = []                                    # (re, im) of every emission since the last Reset
        self.trigger_at = []                             # emission numbers (since the Reset) of the triggers found
        self.display_at = []                             # ... and of the displays
        self.Reset()

    # ------------------------------------------------------------------ slots
    def _skip(self):
        capturesize = (float(self.m_HorzSpan) * self.m_DisplaySampleRate / 1000.0)
        self.m_DisplaySkipValue = c_int(self.m_DisplaySampleRate / (capturesize * self.m_DisplayRate))   # a qint32, testbench.h:174

    def OnDisplayRate(self, rate):                       # :247-254
        self.m_DisplayRate = rate
        self._skip()

    def OnVertRange(self, r):                            # :261-263
        self.m_VertRange = r

    def OnHorzSpan(self, span):                          # :270-279
        self.m_HorzSpan = span
        self._skip()
        self.m_TimeScrnPixel = .001 * (float(self.m_HorzSpan) / float(self.w))

    def OnTriggerMode(self, trigindex):                  # :288-292
        self.m_TrigIndex = trigindex
        self.Reset()

    def OnTrigLevel(self, level):                        # :294-296
        self.m_TrigLevel = level

    def resizeEvent(self, w, h):                         # :920-932
        self.w, self.h = w, h
        self.Reset()

    def Reset(self):                                     # :541-548, :555-565, :574
        self.m_TimeScrnPixel = .001 * (float(self.m_HorzSpan) / float(self.w))
        self.m_TimeScrnPos = 0
        self.m_TimeInPos = 0
        self.m_PreviousSample = 0
        self.m_PostScrnCaptureLength = (7 * self.w) // 10
        self.m_TrigState = TRIGSTATE_WAIT
        for i in range(TB_MAX_SCREENSIZE):
            self.m_TimeBuf1[i] = 0
            self.m_TimeBuf2[i] = 0
        self._skip()
        self.m_DisplaySkipCounter = -2
        self.log, self.trigger_at, self.display_at = [], [], []

    def time_plot_done(self):                            # :995-999
        if self.m_TrigIndex != TRIG_PSINGLE and self.m_TrigIndex != TRIG_NSINGLE:
            self.m_TrigState = TRIGSTATE_WAIT

    # ------------------------------------------------------------------ DisplayData
    def DisplayData(self, re, im, samplerate, on_emit=None):
        """re: the samples (floats); im: the imaginary parts, or None for the real overload (:643-695).
        on_emit(i): called with the index of the sample of every emission (the emission sequence)."""
        if self.m_DisplaySampleRate != samplerate:       # :587-592
            self.m_DisplaySampleRate = samplerate
            self.Reset()                                 # at once (the reference queues ResetSignal)
            return
        w = self.w
        for i in range(len(re)):                         # :614-634
            intime = float(self.m_TimeInPos) / samplerate
            scrntime = float(self.m_TimeScrnPos) * self.m_TimeScrnPixel
            self.m_TimeInPos += 1
            while intime >= scrntime:
                a, b = c_int(re[i]), (c_int(im[i]) if im is not None else 0)
                if on_emit is not None:
                    on_emit(i)
                self.ChkForTrigger(a)
                self.log.append((a, b))
                self.m_TimeBuf1[self.m_TimeScrnPos] = a
                self.m_TimeBuf2[self.m_TimeScrnPos] = b
                self.m_TimeScrnPos += 1
                scrntime = float(self.m_TimeScrnPos) * self.m_TimeScrnPixel
                if self.m_TimeScrnPos >= w:
                    self.m_TimeScrnPos = 0
                    self.m_TimeInPos = 0
                    break

    def ChkForTrigger(self, sample):                     # :819-898
        q = len(self.log)                                # the number of this emission
        if self.m_TrigIndex == TRIG_OFF:
            if 0 == self.m_TimeScrnPos:
                self.m_DisplaySkipCounter += 1
                if self.m_DisplaySkipCounter >= self.m_DisplaySkipValue and self.m_DisplaySkipCounter > 2:
                    self.m_DisplaySkipCounter = 0
                    self.m_TrigBufPos = 0
                    self.m_TrigState = TRIGSTATE_DISPLAY
        elif self.m_TrigIndex in (TRIG_PNORM, TRIG_PSINGLE, TRIG_NNORM, TRIG_NSINGLE):
            if TRIGSTATE_WAIT == self.m_TrigState:
                if self.m_TrigIndex in (TRIG_PNORM, TRIG_PSINGLE):
                    hit = sample >= self.m_TrigLevel and self.m_PreviousSample < self.m_TrigLevel
                else:
                    hit = sample <= self.m_TrigLevel and self.m_PreviousSample > self.m_TrigLevel
                if hit:
                    self.m_TrigBufPos = self.m_TimeScrnPos
                    self.m_TrigState = TRIGSTATE_CAPTURE
                    self.m_TrigCounter = 0
                    self.trigger_at.append(q)
            elif TRIGSTATE_CAPTURE == self.m_TrigState:
                self.m_TrigCounter += 1
                if self.m_TrigCounter >= self.m_PostScrnCaptureLength:
                    self.m_TrigState = TRIGSTATE_DISPLAY
                    self.m_TrigCounter = 0
        if TRIGSTATE_DISPLAY == self.m_TrigState:
            self.m_TrigState = TRIGSTATE_WAITDISPLAY
            w = self.w
            bufpos = self.m_TrigBufPos + self.m_PostScrnCaptureLength - w
            if bufpos < 0:
                bufpos = w + bufpos
            for i in range(w):
                self.m_TimeScrnBuf1[i] = self.m_TimeBuf1[bufpos]
                self.m_TimeScrnBuf2[i] = self.m_TimeBuf2[bufpos]
                bufpos += 1
                if bufpos >= w:
                    bufpos = 0
            self.emits += 1
            self.display_at.append(q)
        self.m_PreviousSample = sample

    # ------------------------------------------------------------------ readers
    def screen(self):
        return self.m_TimeScrnBuf1[:self.w], self.m_TimeScrnBuf2[:self.w]

    def state(self):
        return [self.m_TimeInPos, self.m_TimeScrnPos, self.m_PreviousSample, self.m_TrigState, self.m_TrigCounter,
                self.m_TrigBufPos, self.m_DisplaySkipCounter]

    def vertical(self, v):                               # :973-977 with a 64-bit product
        c = self.h // 2
        return c - c_div(2 * c * v, self.m_VertRange)


def emission_sequence(inpos, pos, pix, sr, w, n):
    """the index of the sample of every emission of n samples from the state (inpos, pos), and the state afterwards:
    the loop of :614-634 alone"""
    out = []
    for i in range(n):
        intime = float(inpos) / sr
        scrntime = float(pos) * pix
        inpos += 1
        while intime >= scrntime:
            out.append(i)
            pos += 1
            scrntime = float(pos) * pix
            if pos >= w:
                pos = 0
                inpos = 0
                break
    return out, pos, inpos


def signal(c, n, cpx=False, seed=1234):
    """row c of the issue: 3000 sin(2 pi 0.0137 i) + uniform noise of +-50 (complex: + j 3000 cos + noise), fp32"""
    import numpy as np
    rng = np.random.default_rng(seed + c)
    i = np.arange(n, dtype=np.float64)
    re = 3000.0 * np.sin(2.0 * math.pi * 0.0137 * i) + rng.uniform(-50.0, 50.0, n)
    if not cpx:
        return re.astype(np.float32)
    im = 3000.0 * np.cos(2.0 * math.pi * 0.0137 * i) + rng.uniform(-50.0, 50.0, n)
    return (re + 1j * im).astype(np.complex64)


# ---------------------------------------------------------------------------------------------------- the scenario
# One object has one screen geometry, so the issue's receivers -- its first five configurations in the modes PNORM,
# NNORM, PNORM, OFF, PSINGLE (a sixth receiver repeats the object's own configuration in NNORM), one level that is
# never reached, one receiver with n = 0 throughout -- are run once per screen width of those five configurations:
# 16 receivers in one object each time, receiver k of the object with configuration k's width being that
# configuration itself.  The rest varies mode, level and display rate.
N_SAMPLES = 20000
MODES5 = [TRIG_PNORM, TRIG_NNORM, TRIG_PNORM, TRIG_OFF, TRIG_PSINGLE]
UNREACHED, IDLE = 6, 7                                   # the receivers with level 5000 and with n = 0


def receivers(k):
    """[(span ms, sample rate, mode, level, display rate)] * 16 for the object with configuration k's width"""
    out = [(CONFIGS[j][1], CONFIGS[j][2], MODES5[j], 100, 10) for j in range(5)]
    _, span, sr = CONFIGS[k]
    out.append((span, sr, TRIG_NNORM, 100, 10))
    out.append((span, sr, TRIG_PNORM, 5000, 10))
    out.append((span, sr, TRIG_PNORM, 100, 10))
    out += [(span, sr, TRIG_NSINGLE, 100, 10), (span, sr, TRIG_PNORM, -2000, 10), (span, sr, TRIG_NNORM, 2900, 10),
            (span, sr, TRIG_OFF, 100, 1), (span, sr, TRIG_OFF, 100, 15), (2 * span + 1, sr, TRIG_PSINGLE, 0, 10),
            (span, 2.0 * sr, TRIG_NNORM, -2999, 10), (max(1, span // 2), sr, TRIG_OFF, 100, 7)]
    assert len(out) == 16
    return out


def cuts(n=N_SAMPLES, seed=99):
    import numpy as np
    rng, out = np.random.default_rng(seed), []
    while sum(out) < n:
        out.append(min(int(rng.choice([1, 7, 256, 513, 1000])), n - sum(out)))
    return out


def configure(dut, k, h=100):
    """dut: anything with the reference's slot names taking (value, channel)"""
    dut.resizeEvent(CONFIGS[k][0], h)
    for c, (span, sr, mode, level, rate) in enumerate(receivers(k)):
        dut.OnHorzSpan(span, c); dut.OnDisplayRate(rate, c); dut.OnTrigLevel(level, c); dut.OnTriggerMode(mode, c)


class RefBatch:
    """16 restatements behind the batch's interface"""

    def __init__(self, channels=16):
        self.r = [RefScope() for _ in range(channels)]

    def resizeEvent(self, w, h):
        for r in self.r:
            r.resizeEvent(w, h)

    def _each(self, name, v, channel):
        for r in (self.r if channel < 0 else [self.r[channel]]):
            getattr(r, name)(*v)

    def OnHorzSpan(self, v, channel=-1): self._each("OnHorzSpan", (v,), channel)
    def OnDisplayRate(self, v, channel=-1): self._each("OnDisplayRate", (v,), channel)
    def OnTrigLevel(self, v, channel=-1): self._each("OnTrigLevel", (v,), channel)
    def OnTriggerMode(self, v, channel=-1): self._each("OnTriggerMode", (v,), channel)
    def OnVertRange(self, v, channel=-1): self._each("OnVertRange", (v,), channel)
    def Reset(self, channel=-1): self._each("Reset", (), channel)
    def time_plot_done(self, channel=-1): self._each("time_plot_done", (), channel)

    def put(self, rows, pos, n, rates):
        """rows: numpy [channels, T] float32 or complex64; samples pos..pos+n[c]-1 of row c; n[c] = 0: not called"""
        for c, r in enumerate(self.r):
            if n[c] == 0:
                continue
            x = rows[c, pos:pos + n[c]]
            if rows.dtype.kind == "c":
                r.DisplayData(x.real.tolist(), x.imag.tolist(), rates[c])
            else:
                r.DisplayData(x.tolist(), None, rates[c])

    def totals(self):
        return [r.emits for r in self.r]

    def screen(self, c):
        return self.r[c].screen()

    def state(self, c):
        return self.r[c].state()


def run(dut, rows, k, call_cuts, events=None, idle=(IDLE,), record=None):
    """Feeds rows to dut in call_cuts with configuration k's receivers' rates; events: {call index: [(channel, name,
    value)]}, name a slot or "rate".  After every call record(i, emits) is called with the emits of the call (dut is a
    RefBatch, whose totals are differenced here)."""
    rates = [r[1] for r in receivers(k)]
    pos, seen = 0, dut.totals()
    for i, n in enumerate(call_cuts):
        for c, name, v in (events or {}).get(i, ()):
            if name == "rate":
                rates[c] = v
            elif v is None:
                getattr(dut, name)(c)
            else:
                getattr(dut, name)(v, c)
        ns = [0 if c in idle else n for c in range(len(rates))]
        dut.put(rows, pos, ns, rates)
        pos += n
        now = dut.totals()
        emits = [a - b for a, b in zip(now, seen)]
        seen = now
        if record is not None:
            record(i, emits)
        for c, e in enumerate(emits):
            if e:
                dut.time_plot_done(c)


_TRACES = {}


def trace(k, cpx, events_key=None, events=None, call_cuts=None):
    """the restatement over the scenario, computed once: [(emits of the call, {c: screen of every receiver that
    emitted})] per call, the final states and the totals"""
    key = (k, cpx, events_key, tuple(call_cuts) if call_cuts else None)
    if key not in _TRACES:
        import numpy as np
        rows = np.stack([signal(c, N_SAMPLES, cpx) for c in range(16)])
        ref = RefBatch()
        configure(ref, k)
        calls = []
        run(ref, rows, k, call_cuts or cuts(), events,
            record=lambda i, emits: calls.append((emits, {c: ref.screen(c) for c, e in enumerate(emits) if e})))
        _TRACES[key] = (rows, calls, [ref.state(c) for c in range(16)], ref.totals(), [ref.screen(c) for c in range(16)])
    return _TRACES[key]


def check(dut, k, cpx, events_key=None, events=None, call_cuts=None):
    """dut (configured here) over the scenario against the restatement: the emits of every call, the screen of every
    receiver whenever it emitted, and at the end every receiver's state and screen.  Returns the restatement's totals."""
    rows, calls, states, totals, screens = trace(k, cpx, events_key, events, call_cuts)
    configure(dut, k)

    def record(i, emits):
        assert emits == calls[i][0], (i, emits, calls[i][0])
        for c, scr in calls[i][1].items():
            assert dut.screen(c) == scr, (i, c)

    run(dut, rows, k, call_cuts or cuts(), events, record=record)
    dut.put(rows, 0, [0] * 16, [r[1] for r in receivers(k)])                    # a put of nothing applies the last time_plot_done
    for c in range(16):
        assert dut.state(c) == states[c], (c, dut.state(c), states[c])
        assert dut.screen(c) == screens[c], c
    return totals


def check_counts(k, totals):
    """the run is not vacuous: the object's own configuration displayed as its mode says (NORM at least 3 screens, the
    single one exactly 1, TRIG_OFF at least 2), the unreachable level never, the idle receiver never"""
    mode = MODES5[k]
    if mode in (TRIG_PNORM, TRIG_NNORM):
        assert totals[k] >= 3, totals
    elif mode == TRIG_PSINGLE:
        assert totals[k] == 1, totals
    else:
        assert totals[k] >= 2, totals
    assert totals[5] >= 3, totals                        # the own configuration in NNORM
    assert totals[UNREACHED] == 0 and totals[IDLE] == 0, totals


# slots in mid-stream (call index: channel, name, value): a span change in mid-sweep, a level change, a mode change (a
# reset) and a sample-rate change (drops that call and resets); "rate" changes the rate the calls carry from then on
def mid_stream_events(k):
    span, sr = CONFIGS[k][1], CONFIGS[k][2]
    return {5: [(0, "OnHorzSpan", 2 * span + 3), (9, "OnHorzSpan", max(1, span // 2))],
            9: [(2, "OnTrigLevel", -1500), (5, "OnTrigLevel", 1200)],
            14: [(1, "OnTriggerMode", TRIG_PNORM), (3, "OnTriggerMode", TRIG_NSINGLE), (12, "OnTriggerMode", TRIG_NNORM)],
            20: [(4, "rate", 2.0 * CONFIGS[4][2]), (5, "rate", 0.5 * sr), (11, "rate", 3.0 * sr)],
            26: [(8, "Reset", None), (11, "OnDisplayRate", 15), (10, "OnHorzSpan", 3 * span)],
            31: [(6, "OnTrigLevel", 2000)]}
