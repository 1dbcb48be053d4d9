"""The FFT view of the batch test-bench scope on the device (csdr_scope_batch after set_time_display(..., 0), K10)
against scope_fft_ref.py, the restatement of the reference's frequency branch (gui/testbench.cpp:594-611, :654-672,
:1005-1068) around the fp64 oracle's CFft.

Counts, emits, get_fft_state, skip values and positions are integers and exact.  Bels: assert_spectrum_close of
tests/test_fft_resampler_gpu.py against the oracle's m_pFFTAveBuf of the same frame.  Pixels: that function's three
classes give each bin a tolerance; the restatement's mapping run on bels + tol and on bels - tol gives an interval per
pixel (mapping and per-pixel minimum are monotone), lo <= got <= hi; the peak's interval is the running minimum of the
draws' lo and hi.  assert_spectrum_close says nothing at or below -15 bels, so every test asserts on the oracle alone
that no bin of a used frame is that low: the inputs are tones at -20 and -30.5 dBFS plus Gaussian noise at -40 dBFS.

8 receivers, at most 40 frames (81 920 samples) each, in calls cut from {1, 7, 256, 513, 2048, 2049, 5000}."""
import numpy as np
import pytest

import scope_fft_ref as F
import scope_ref as R
from test_fft_resampler_gpu import assert_spectrum_close

pytestmark = pytest.mark.gpu

CH, IDLE, TOTAL = 8, 5, 40 * 2048
# (sample rate, display rate): skip values 3, 1, 0, 2, 0, (idle), 1, 3
RX = [(62500.0, 10), (62500.0, 20), (62500.0, 100), (48001.0, 10), (12345.0, 3), (62500.0, 10), (8000.0, 2), (204800.0, 30)]
SKIPS = [3, 1, 0, 2, 2, 0, 1, 3]                         # (the idle receiver never learns its rate: 1 / 20480)


def cuts(seed=7):
    """The calls: the first carries the new rate and is dropped; then (positions count from there) eight of 256 -- the
    eighth ends exactly on a frame boundary, its frame gathered in the carry --, 513, 513, 256 -- each wholly inside a
    frame --, 5000 -- spans three frames, the first begun in the carry --, a 1 and a 7; the rest drawn at random."""
    out = [513] + [256] * 8 + [513, 513, 256, 5000, 1, 7]
    rng = np.random.default_rng(seed)
    while True:
        k = int(rng.choice([1, 7, 256, 513, 2048, 2049, 5000]))
        if sum(out) + k > TOTAL:
            return out
        out.append(k)


def test_the_cuts_are_as_described():
    c = cuts()
    assert set(c) == {1, 7, 256, 513, 2048, 2049, 5000} and sum(c) <= TOTAL
    pos, inside, boundary, three = 0, False, False, False
    for n in c[1:]:
        frames = (pos + n) // 2048
        inside |= frames == 0 and pos > 0
        boundary |= frames >= 1 and (pos + n) % 2048 == 0
        three |= frames >= 3 and pos > 0
        pos = (pos + n) % 2048
    assert inside and boundary and three


def rows_for(cpx, time_view=()):
    """the FFT view's feed; a time-view receiver gets scope_ref's triggering sine"""
    dt = np.complex64 if cpx else np.float32
    x = np.zeros((CH, TOTAL), dtype=dt)
    for c in range(CH):
        x[c] = R.signal(c, TOTAL, cpx) if c in time_view else F.feed_signal(c, TOTAL, RX[c][0], cpx)
    return x


class Gpu:
    """cutesdr_amd.ScopeBatch behind the interface the driver below uses"""

    def __init__(self, channels=CH):
        import torch
        import cutesdr_amd as ca
        torch.cuda.init()
        self.s = ca.ScopeBatch(channels)
        self.t = self.src = None
        for name in ("resizeEvent", "OnHorzSpan", "OnDisplayRate", "OnTriggerMode", "OnTrigLevel", "Reset", "time_plot_done",
                     "OnTimeDisplay", "OnEnablePeak"):
            setattr(self, name, getattr(self.s, name))

    def put(self, rows, pos, n, rates):
        import torch
        if self.src is not rows:
            self.src, self.t = rows, torch.from_numpy(rows).cuda()
            self.before = self.t.clone()
        self.s.DisplayData(self.t, n, rates, offset=pos)


def check_fft(s, c, r, what):
    """bels, screen and peak of receiver c against the restatement r, as under Tolerances"""
    assert_spectrum_close(s.get_fft_ave(c).astype(np.float64), r.bels)
    scr, pk, cpx = s.get_fft_screen(c)
    w = r.w
    assert cpx == r.fft_cpx, what
    assert (r.scr_lo <= scr).all() and (scr <= r.scr_hi).all(), (what, np.abs(scr - np.array(r.fft_screen[:w])).max())
    assert (r.pk_lo[:w] <= pk).all() and (pk <= r.pk_hi[:w]).all(), (what, np.abs(pk - np.array(r.m_FftPkBuf[:w])).max())


def drive(d, ref, rows, call_cuts, rates, events=None, idle=(IDLE,), after_call=None):
    """The same calls and events into the device d and the restatement batch ref.  After every call: the emits of every
    receiver and get_fft_state of every FFT-view receiver, exact; of each FFT-view receiver that emitted bels, screen
    and peak; of every time-view receiver state and screen, exact, and time_plot_done where it emitted.  The same
    again at the end.  events: {call index: [(channel, slot name or "rate", value)]}."""
    rates = list(rates)
    pos, seen, drawn = 0, [0] * len(ref.r), 0
    cpx = rows.dtype.kind == "c"

    def compare(c, r, emitted, what):
        if r.m_TimeDisplay:
            assert d.s.get_state(c)[:7].tolist() == r.state(), what
            re, im = d.s.get_screen(c)
            assert (re.tolist(), im.tolist()) == r.screen(), what
        else:
            assert d.s.get_fft_state(c).tolist() == r.fft_state(), (what, d.s.get_fft_state(c).tolist(), r.fft_state())
            if emitted:
                check_fft(d.s, c, r, what)

    for i, n in enumerate(call_cuts):
        for c, name, v in (events or {}).get(i, ()):
            if name == "rate":
                rates[c] = v
            else:
                for x in (d, ref):
                    getattr(x, name)(c) if v is None else getattr(x, name)(v, c)
        ns = [0 if c in idle else n for c in range(len(rates))]
        d.put(rows, pos, ns, rates)
        ref.put(rows, pos, ns, rates)
        pos += n
        emits = d.s.get_emits().tolist()
        want = [r.emits - a for r, a in zip(ref.r, seen)]
        seen = [r.emits for r in ref.r]
        assert emits == want, (i, emits, want)
        for c, r in enumerate(ref.r):
            compare(c, r, emits[c] > 0, (i, c))
            if r.m_TimeDisplay and emits[c]:
                d.time_plot_done(c); ref.time_plot_done(c)
            if not r.m_TimeDisplay:
                F.assert_above_floor(r.draws)
                drawn += len(r.draws)
                r.draws = []
        if after_call is not None:
            after_call(i)
    for c, r in enumerate(ref.r):
        compare(c, r, r.total > 0 and not r.m_TimeDisplay, ("end", c))
    return drawn


def configure(x, w, h, fft=range(CH)):
    x.resizeEvent(w, h)
    for c in range(CH):
        x.OnDisplayRate(RX[c][1], c)
        if c in fft:
            x.OnTimeDisplay(False, c)


# ------------------------------------------------------------------------------------------------- 1 parity
@pytest.mark.parametrize("w,h", [(100, 100), (700, 255), (2048, 300)])
@pytest.mark.parametrize("cpx", [False, True], ids=["real", "complex"])
def test_parity(oracle, cpx, w, h):
    d, ref = Gpu(), F.RefFftBatch(oracle, CH)
    configure(d, w, h); configure(ref, w, h)
    assert [r.m_DisplaySkipValue for r in ref.r] != SKIPS                       # not yet: the rate is still 1
    drawn = drive(d, ref, rows_for(cpx), cuts(), [r[0] for r in RX])
    assert [r.m_DisplaySkipValue for r in ref.r] == SKIPS and {0, 1, 3} <= set(SKIPS)
    assert drawn >= 60 and all(r.total >= 5 for c, r in enumerate(ref.r) if c != IDLE), drawn
    assert ref.r[IDLE].total == 0 and d.s.get_fft_state(IDLE).tolist()[3] == 0


# ------------------------------------------------------------------------------------------------- 2 the cut
@pytest.mark.parametrize("cpx", [False, True], ids=["real", "complex"])
def test_cut_does_not_matter_bit_for_bit(cpx):
    """one call of the whole stream against the uneven calls: identical bels, screen, peak and state; the first call,
    carrying the new rate, is dropped in both"""
    rows, rates, c = rows_for(cpx), [r[0] for r in RX], cuts()
    out = []
    for call_cuts in (c, [c[0], sum(c) - c[0]]):
        d = Gpu()
        configure(d, 700, 255)
        pos = 0
        for n in call_cuts:
            d.put(rows, pos, [0 if k == IDLE else n for k in range(CH)], rates)
            pos += n
        out.append([(d.s.get_fft_ave(k).view(np.uint32).tolist(), d.s.get_fft_screen(k)[0].tolist(), d.s.get_fft_screen(k)[1].tolist(),
                     d.s.get_fft_state(k).tolist()) for k in range(CH)])
    assert out[0] == out[1]
    assert all(out[0][k][3][3] >= 5 for k in range(CH) if k != IDLE) and out[0][IDLE][3] == [0, -2, SKIPS[IDLE], 0]


# ------------------------------------------------------------------------------------------------- 3 events
def test_mid_stream_events(oracle):
    """OnDisplayRate; a changed sample rate (drops the call, resets, peak back to h); Reset in mid-frame; OnEnablePeak
    on an FFT-view receiver and on a time-view one (its ring is zeroed; its later screens equal the wrapped scope_ref
    exactly); OnTimeDisplay to the other view and back -- against the restatement given the same events"""
    w, h, tv = 100, 100, (4, 6)
    d, ref = Gpu(), F.RefFftBatch(oracle, CH)
    rates = [r[0] for r in RX]
    rates[4], rates[6] = 48000.0, 48000.0
    for x in (d, ref):
        configure(x, w, h, fft=[c for c in range(CH) if c not in tv])
        for c in tv:
            x.OnHorzSpan(10, c); x.OnTriggerMode(R.TRIG_PNORM if c == 4 else R.TRIG_OFF, c)
    ev = {8: [(0, "OnDisplayRate", 100)],
          13: [(1, "rate", 31250.0)],
          16: [(2, "Reset", None)],
          18: [(3, "OnEnablePeak", True), (4, "OnEnablePeak", True), (6, "OnEnablePeak", False)],
          20: [(7, "OnTimeDisplay", True), (6, "OnTimeDisplay", False)],
          24: [(7, "OnTimeDisplay", False), (6, "OnTimeDisplay", True)]}
    seen = {}

    def after_call(i):
        if i == 12:
            seen["pk1"] = d.s.get_fft_screen(1)[1].tolist()
        if i == 13:                                      # the call with the new rate: nothing used, peak back to h
            assert seen["pk1"] != [h] * w and d.s.get_fft_screen(1)[1].tolist() == [h] * w
            assert d.s.get_fft_state(1).tolist() == [0, -2, R.c_int(31250.0 / 20480 / 2), 0]
        if i == 17:
            seen["ring"] = list(ref.r[4].m_TimeBuf1[:w])
        if i == 18:
            assert d.s.get_fft_screen(3)[1].tolist() != [h] * w or ref.r[3].draws == []

    c = cuts()
    assert max(ev) < len(c) - 4
    drawn = drive(d, ref, rows_for(False, time_view=tv), c, rates, ev, after_call=after_call)
    assert any(seen["ring"]) and drawn >= 30
    assert ref.r[4].emits >= 2 and ref.r[6].emits >= 1 and ref.r[7].total >= 1


# ------------------------------------------------------------------------------------------------- 4 mixed object
def test_mixed_views_and_non_interference(oracle):
    import torch
    w, h, tv = 700, 255, (1, 3, 6, 7)
    d, ref = Gpu(), F.RefFftBatch(oracle, CH)
    rates = [48000.0 if c in tv else RX[c][0] for c in range(CH)]
    for x in (d, ref):
        configure(x, w, h, fft=[c for c in range(CH) if c not in tv])
        for c in tv:
            x.OnHorzSpan(10 + c, c); x.OnTriggerMode([R.TRIG_PNORM, R.TRIG_NNORM, R.TRIG_OFF, R.TRIG_PSINGLE][tv.index(c)], c)
    rows = rows_for(True, time_view=tv)
    d.put(rows, 0, [0] * CH, rates); ref.put(rows, 0, [0] * CH, rates)            # the settings alone
    idle0 = (d.s.get_fft_state(IDLE).tolist(), [a.tolist() for a in d.s.get_fft_screen(IDLE)[:2]], d.s.get_state(IDLE).tolist())
    assert idle0[0] == [0, -2, 0, 0] and idle0[1] == [[0] * w, [h] * w]
    drawn = drive(d, ref, rows, cuts(), rates)
    torch.cuda.synchronize()
    assert drawn >= 30 and all(ref.r[c].emits >= 1 for c in tv)
    assert torch.equal(torch.view_as_real(d.t).view(torch.int32), torch.view_as_real(d.before).view(torch.int32))   # the input rows
    assert (d.s.get_fft_state(IDLE).tolist(), [a.tolist() for a in d.s.get_fft_screen(IDLE)[:2]], d.s.get_state(IDLE).tolist()) == idle0
    out = torch.empty((CH + 1, 2, w + 5), dtype=torch.int32, device="cuda")
    out.copy_((torch.arange(out.numel(), device="cuda", dtype=torch.int64) * 2654435761 % 2147483647).to(torch.int32).view(out.shape))
    pat = out.clone()
    d.s.get_fft_screens_all(out)
    torch.cuda.synchronize()
    assert torch.equal(out[:CH, :, w:], pat[:CH, :, w:]) and torch.equal(out[CH], pat[CH])
    o = out.cpu().numpy()
    for c in range(CH):
        if c in tv:
            assert torch.equal(out[c], pat[c]), c
        else:
            scr, pk, _ = d.s.get_fft_screen(c)
            assert o[c, 0, :w].tolist() == scr.tolist() and o[c, 1, :w].tolist() == pk.tolist(), c


# ------------------------------------------------------------------------------------------------- 5 anchor
def test_anchor_tone():
    """Not through the restatement: a tone at exactly fs/8, -20 dBFS, on a 2048-wide screen, fs = 204800 (m_Span =
    204800).  Complex: bin 1024 + 256 = 1280 at -1.3982 bels (SURVEY 8c's anchor; K_B normalises by N A / 2), +- 0.001.
    The issue places the smallest y at pixel 1280, "one bin per pixel"; the reference's translate table says otherwise:
    m_BinMax is clamped to 2047 (dsp/fft.cpp:344-345), so 2047 bins spread over 2048 pixels, pixel x shows bin
    (x * 2047) / 2048 = x - 1, and bin 1280 sits at pixel 1281 (the oracle's GetScreenIntegerFFTData agrees); pixel 1280
    shows bin 1279, the window's -6.02 dB skirt.  As a real row the tone's two lines are 6.02 dB lower, -2.0003 bels;
    start = 0 gives m_BinMin = 1024, 1023 bins over 2048 pixels, pixel x shows bin 1024 + (x * 1023) / 2048: bin 1280
    at pixels 513 and 514.  y = (int)(h * (-10 / 180) * (bels - 1)), h = 300."""
    from util_signals import FULL_SCALE
    fs, w, h = 204800.0, 2048, 300
    t = np.arange(4 * 2048, dtype=np.float64)
    z = FULL_SCALE * 0.1 * np.exp(2j * np.pi * t / 8.0)
    level = lambda bels: [int(h / 18.0 * (1.0 - (bels + s))) for s in (0.001, -0.001)]

    def run(x):
        d = Gpu(1)
        d.resizeEvent(w, h); d.OnTimeDisplay(False); d.OnDisplayRate(1000)
        rows = x.reshape(1, -1)
        d.put(rows, 0, [1], [fs])                        # the new rate
        d.put(rows, 0, [len(x)], [fs])
        assert d.s.get_emits().tolist() == [3] and d.s.get_fft_state(0).tolist() == [0, 0, 0, 3]
        return d.s.get_fft_screen(0), d.s.get_fft_ave(0)

    (scr, pk, cpx), bels = run(z.astype(np.complex64))
    assert cpx and np.argmax(bels) == 1280 and abs(float(bels[1280]) + 1.3982) <= 0.001
    assert [x for x in range(w) if (x * 2047) // 2048 == 1280] == [1281]
    lo, hi = level(-1.3982)
    assert np.flatnonzero(scr == scr.min()).tolist() == [1281] and lo <= scr[1281] <= hi and pk.tolist() == scr.tolist()
    lo6, hi6 = level(-1.3982 - 0.60206)
    assert lo6 <= scr[1280] <= hi6 and lo6 <= scr[1282] <= hi6

    (scr, pk, cpx), bels = run(z.real.astype(np.float32))
    px = [x for x in range(w) if 1024 + (x * 1023) // 2048 == 1280]
    assert not cpx and px == [513, 514]
    lo, hi = level(-1.3982 - 0.60206)
    assert np.flatnonzero(scr == scr.min()).tolist() == px and lo <= scr[513] <= hi


# ------------------------------------------------------------------------------------------------- 6 the whole bench
def test_generator_sweep_paints_the_peak_trace():
    """TestGenBatch straight into put_cpx: a -10 dBFS tone from f1 = -8 kHz to f2 = +8 kHz across six calls of 13648
    samples at 204.8 kS/s (39 frames, every one after the first drawn: display rate 200, skip value 0).  The scope
    drops the first call (the new rate) and never uses the first complete frame after a reset, so the tone stands at
    f1 for the first two calls (sweep rate 0); the sweep then runs at 100 kHz/s -- 10 bins per frame, so no frequency
    is passed only under the window's zeros -- and reaches f2 during the fifth call, where the generator stops it
    (:426-427).  Afterwards the peak trace is strong, y below the level of -40 dBFS = (int)(h * 5 / 18), on every
    pixel between those of f1 and f2, and the last screen is strong only within 3 pixels of f2's."""
    import torch
    import cutesdr_amd as ca
    fs, T, w, h = 204800.0, 13648, 700, 255
    f1, f2, rate = -8000.0, 8000.0, 100000.0
    g = ca.TestGenBatch(2)
    g.OnGenOn(True); g.OnSweepStart(f1); g.OnSweepStop(f2); g.OnSweepRate(0.0); g.OnSignalPwr(-10.0); g.OnNoisePwr(-70.0)
    g.OnPulseWidth(0.0)                                  # no gating (the constructor's 10 ms of every 500, :119-120)
    s = ca.ScopeBatch(2)
    s.resizeEvent(w, h); s.OnTimeDisplay(False); s.OnDisplayRate(200)
    rows = torch.zeros((2, T), dtype=torch.complex64, device="cuda")
    for i in range(6):
        if i == 2:
            g.OnSweepRate(rate)
        g.CreateGeneratorSamples(rows, T, fs)
        s.DisplayData(rows, T, fs)
    assert s.get_emits().tolist() == [5 * T // 2048 - 1] * 2 and (f2 - f1) / rate < 2.9 * T / fs
    pixel = lambda f: ((int(f * 2048 / fs) + 1024 - 0) * w) // 2047          # m_BinMin = 0, m_BinMax = 2047: the bins branch
    p1, p2, strong = pixel(f1), pixel(f2), int(h * 5.0 / 18.0)
    assert p2 - p1 >= 50
    for c in range(2):
        scr, pk, cpx = s.get_fft_screen(c)
        assert cpx and (pk[p1:p2 + 1] < strong).all(), np.flatnonzero(pk[p1:p2 + 1] >= strong)
        on = np.flatnonzero(scr < strong)
        assert len(on) >= 1 and on.min() >= p2 - 3 and on.max() <= p2 + 3, on


# ------------------------------------------------------------------------------------------------- 7 bad arguments
def test_rejects_bad_arguments():
    import ctypes as C
    import torch
    import cutesdr_amd as ca
    from cutesdr_amd._capi import lib, CSDR_EINVAL
    rows = torch.zeros((2, 4096), dtype=torch.float32, device="cuda")
    s = ca.ScopeBatch(2)
    s.OnTimeDisplay(False, 0)
    s.DisplayData(rows, [1, 1], [48000.0, 48000.0])
    s.DisplayData(rows, [3000, 3000], [48000.0, 48000.0])
    state = lambda: ([s.get_fft_state(c).tolist() for c in range(2)], [s.get_state(c).tolist() for c in range(2)])
    s0 = state()
    assert s0[0][0][0] == 3000 - 2048
    with pytest.raises(ca._capi.CsdrError):
        s.put_ptr(rows.data_ptr(), 4096, [100, 100], [2.0 ** 31, 48000.0])      # a rate of 2^31 in the FFT view
    s.put_ptr(rows.data_ptr(), 4096, [0, 0], [2.0 ** 31, 2.0 ** 31])            # ... is not looked at where n = 0
    with pytest.raises(ca._capi.CsdrError):
        s.put_ptr(rows.data_ptr(), 64, [65, 0], 48000.0)                        # n > stride
    buf = np.zeros(2048, dtype=np.int32)
    p = C.c_void_p(buf.ctypes.data)
    assert lib().csdr_scope_batch_get_fft_screen(s.h, 0, None, p) == CSDR_EINVAL
    assert lib().csdr_scope_batch_get_fft_screen(s.h, 0, p, None) == CSDR_EINVAL
    assert lib().csdr_scope_batch_get_fft_ave(s.h, 0, None) == CSDR_EINVAL
    assert lib().csdr_scope_batch_get_fft_state(s.h, 0, None) == CSDR_EINVAL
    assert lib().csdr_scope_batch_get_fft_screens_all(s.h, None, 100, None) == CSDR_EINVAL
    out = torch.zeros((2, 2, 100), dtype=torch.int32, device="cuda")
    assert lib().csdr_scope_batch_get_fft_screens_all(s.h, C.c_void_p(out.data_ptr()), 99, None) == CSDR_EINVAL   # out_stride < w
    assert state() == s0
    s.DisplayData(rows, [100, 100], [48000.0, 48000.0])                          # the rate is still the last good call's
    assert s.get_fft_state(0).tolist()[0] == 3100 - 2048
