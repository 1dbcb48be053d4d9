"""The batch test-bench scope on the device (csdr_scope_batch, K10) against scope_ref.py, the line-for-line restatement
of the time view of the reference's test bench (gui/testbench.cpp:583-695, :819-898, :973-999).  Every comparison is
on integers and exact.

The scenario (scope_ref.py): 16 receivers in one object, rows 3000 sin(2 pi 0.0137 i) + uniform noise of +-50 (complex:
+ j 3000 cos), 20000 samples per receiver in uneven calls drawn from {1, 7, 256, 513, 1000}.  An object has one screen
geometry, so the scenario runs once per screen width of the issue's first five configurations (w, span, rate), the
receivers of each object being those five (span, rate) in the modes PNORM, NNORM, PNORM, OFF, PSINGLE, the object's own
configuration again in NNORM, a level that is never reached, a receiver with n = 0 throughout, and eight more that
vary mode, level and display rate."""
import numpy as np
import pytest

import scope_ref as R

pytestmark = pytest.mark.gpu


class GpuBatch:
    """cutesdr_amd.ScopeBatch behind the interface scope_ref.run drives"""

    def __init__(self, channels=16):
        import torch                                     # before the library, as everywhere in this suite
        import cutesdr_amd as ca
        torch.cuda.init()
        self.s = ca.ScopeBatch(channels)
        self.t, self.src = None, None
        self.total = np.zeros(channels, dtype=np.int64)
        for name in ("resizeEvent", "OnHorzSpan", "OnDisplayRate", "OnTriggerMode", "OnTrigLevel", "OnVertRange", "Reset",
                     "time_plot_done"):
            setattr(self, name, getattr(self.s, name))

    def put(self, rows, pos, n, rates):
        import torch
        if self.src is not rows:
            self.src, self.t = rows, torch.from_numpy(rows).cuda()
            self.before = self.t.clone()
        self.s.DisplayData(self.t, n, rates, offset=pos)

    def totals(self):
        self.total += self.s.get_emits()
        return self.total.tolist()

    def screen(self, c):
        re, im = self.s.get_screen(c)
        return re.tolist(), im.tolist()

    def state(self, c):
        return self.s.get_state(c)[:7].tolist()


# ------------------------------------------------------------------------------------------------- 1, 2 parity
@pytest.mark.parametrize("k", range(5))
def test_parity_real(k):
    """after every call the emits of every receiver and the screen of every receiver that emitted, at the end every
    state and screen; time_plot_done for the receivers that emitted, in both"""
    totals = R.check(GpuBatch(), k, False)
    print("screens of the 16 receivers, width %d:" % R.CONFIGS[k][0], totals)
    R.check_counts(k, totals)


@pytest.mark.parametrize("k", range(5))
def test_parity_complex(k):
    """the same with complex rows: both screen halves"""
    d = GpuBatch()
    totals = R.check(d, k, True)
    R.check_counts(k, totals)
    assert any(any(d.screen(c)[1]) for c in range(16))


# ------------------------------------------------------------------------------------------------- 3 the cut
@pytest.mark.parametrize("k", [3, 4], ids=["TRIG_OFF", "PSINGLE"])
def test_cut_does_not_matter(k):
    """one call of the whole stream against the uneven calls: the final screen and the emit count of the TRIG_OFF
    receiver (k = 3) and of the PSINGLE one (k = 4); the first call carries the new rate and is dropped in both"""
    rows, calls, states, totals, screens = R.trace(k, False)
    one = GpuBatch()
    R.configure(one, k)
    first = R.cuts()[0]
    R.run(one, rows, k, [first, R.N_SAMPLES - first])
    assert one.totals()[k] == totals[k] and totals[k] >= 1
    assert one.screen(k) == screens[k]


# ------------------------------------------------------------------------------------------------- 4 non-interference
def test_non_interference():
    import torch
    k = 0
    d = GpuBatch()
    rows, calls, states, totals, screens = R.trace(k, True)
    R.configure(d, k)
    d.put(rows, 0, [0] * 16, [r[1] for r in R.receivers(k)])                    # the settings alone
    idle0 = (d.state(R.IDLE), d.screen(R.IDLE))
    R.run(d, rows, k, R.cuts())
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(d.t).view(torch.int32), torch.view_as_real(d.before).view(torch.int32))   # the input rows
    assert (d.state(R.IDLE), d.screen(R.IDLE)) == idle0 and d.totals()[R.IDLE] == 0
    assert idle0[0] == [0, 0, 0, 0, 0, 0, -2] and not any(idle0[1][0]) and not any(idle0[1][1])
    w = R.CONFIGS[k][0]
    out = torch.empty((17, 2, w + 5), dtype=torch.int32, device="cuda")
    out.copy_((torch.arange(out.numel(), device="cuda", dtype=torch.int64) * 2654435761 % 2147483647).to(torch.int32).view(out.shape))
    pat = out.clone()
    d.s.get_screens_all(out)
    torch.cuda.synchronize()
    assert torch.equal(out[:16, :, w:], pat[:16, :, w:]) and torch.equal(out[16], pat[16])
    o = out.cpu().numpy()
    for c in range(16):
        assert (o[c, 0, :w].tolist(), o[c, 1, :w].tolist()) == d.screen(c) == screens[c], c


# ------------------------------------------------------------------------------------------------- 5 slots in mid-stream
@pytest.mark.parametrize("k", [0, 3])
def test_slots_in_mid_stream(k):
    """a span change in mid-sweep, a level change, a mode change (a reset), a sample-rate change (drops that call and
    resets), a reset and a display-rate change between two calls, against the restatement given the same events"""
    R.check(GpuBatch(), k, False, "mid", R.mid_stream_events(k))


# ------------------------------------------------------------------------------------------------- 6 vertical mapping
@pytest.mark.parametrize("h", [100, 101])
def test_vertical_mapping(h):
    """y = h/2 - (2*(h/2)*v) / m_VertRange with C's truncating division, ranges 65000 and 7, both halves"""
    import torch
    k, w = 0, R.CONFIGS[0][0]
    d = GpuBatch()
    rows, calls, states, totals, screens = R.trace(k, True)
    R.configure(d, k)
    d.s.resizeEvent(w, h)                                # a reset of every receiver, as configure's own
    for c in range(16):
        d.s.OnVertRange(7 if c % 2 else 65000, c)
    R.run(d, rows, k, [R.cuts()[0], 6000])
    out = torch.zeros((16, 2, w), dtype=torch.int32, device="cuda")
    y = torch.full((16, 2, w + 3), -77, dtype=torch.int32, device="cuda")
    d.s.get_screens_all(out, y)
    torch.cuda.synchronize()
    o, yy = out.cpu().numpy(), y.cpu().numpy()
    assert (yy[:, :, w:] == -77).all() and np.abs(o).max() > 1000
    for c in range(16):
        vr = 7 if c % 2 else 65000
        for half in range(2):
            want = [h // 2 - R.c_div(2 * (h // 2) * int(v), vr) for v in o[c, half]]
            assert yy[c, half, :w].tolist() == want, (c, half)


# ------------------------------------------------------------------------------------------------- 7 the whole test bench
def test_round_trip_generator_chain_scope():
    """TestGenBatch (pulse gating on, 4 receivers) -> DemodBatch (AM, strict mode) -> ScopeBatch.put_real in PNORM over
    a few calls of the chain: the screens equal the restatement run on the downloaded audio rows, and on every screen
    the trigger pixel sits at w - Post: screen[w-Post] >= level > screen[w-Post-1].  The level of a receiver is the
    middle of its first audio call, so that the gated carrier crosses it."""
    import torch
    import cutesdr_amd as ca
    from test_postchain_gpu import MODES, info
    C, T, fs, w, calls = 4, 1 << 16, 2.0e6, 100, 6
    post = (7 * w) // 10
    cap = T // 8 + 2048 + 4096
    rows = torch.zeros((C, T), dtype=torch.complex64, device="cuda")
    out = torch.zeros((C, cap), dtype=torch.float32, device="cuda")
    g = ca.TestGenBatch(C)
    g.OnGenOn(True); g.OnSweepRate(0.0); g.OnSignalPwr(-10.0); g.OnNoisePwr(-70.0)
    g.OnPulseWidth(0.002); g.OnPulsePeriod(0.005)
    for c in range(C):
        g.OnSweepStart(100e3 + 300.0 * c, channel=c); g.OnSweepStop(100e3 + 300.0 * c, channel=c)
    b = ca.DemodBatch(C, 2048); b.set_input_rate(fs)
    m, kw = MODES["AM"]
    for c in range(C):
        b.set_demod(c, m, info(ca, **kw))
    b.commit()
    for c in range(C):
        b.set_freq(c, -100e3)
    s = ca.ScopeBatch(C)
    ref = R.RefBatch(C)
    for x in (s, ref):
        x.resizeEvent(w, 100); x.OnHorzSpan(20); x.OnTriggerMode(R.TRIG_PNORM)
    stream = torch.cuda.current_stream().cuda_stream
    shown, levels, seen = 0, None, [0] * C
    for i in range(calls):
        g.CreateGeneratorSamples(rows, T, fs)
        b.process_ptr(rows.data_ptr(), rows.stride(0), T, out.data_ptr(), cap, stream)
        torch.cuda.synchronize()
        n = [b.out_count(c) for c in range(C)]
        rates = [b.output_rate(c) for c in range(C)]
        audio = out.cpu().numpy()
        assert min(n) > 0
        if levels is None:
            levels = [int((float(audio[c, n[c] // 2:n[c]].max()) + float(audio[c, n[c] // 2:n[c]].min())) / 2.0) for c in range(C)]
            for c in range(C):
                s.OnTrigLevel(levels[c], c); ref.OnTrigLevel(levels[c], c)
        s.DisplayData(out, n, rates)
        ref.put(audio, 0, n, rates)
        emits = s.get_emits().tolist()
        assert emits == [r.emits - a for r, a in zip(ref.r, seen)], (i, emits)
        seen = [r.emits for r in ref.r]
        for c in range(C):
            if emits[c]:
                re, im = s.get_screen(c)
                assert (re.tolist(), im.tolist()) == ref.screen(c), (i, c)
                assert re[w - post] >= levels[c] > re[w - post - 1], (i, c, levels[c])
                shown += 1
                s.time_plot_done(c); ref.time_plot_done(c)
    assert shown >= C, shown


def test_rejects_bad_arguments():
    import torch
    import cutesdr_amd as ca
    rows = torch.zeros((2, 64), dtype=torch.float32, device="cuda")
    s = ca.ScopeBatch(2)
    with pytest.raises(ca._capi.CsdrError):
        s.resizeEvent(2049, 100)
    with pytest.raises(ca._capi.CsdrError):
        s.OnTriggerMode(5)
    with pytest.raises(ca._capi.CsdrError):
        s.put_ptr(rows.data_ptr(), 64, [65, 0], 48000.0)                        # n > stride
    with pytest.raises(ca._capi.CsdrError):
        s.put_ptr(rows.data_ptr(), 64, 64, [48000.0, 0.0])                      # a rate of 0
    s.DisplayData(rows, [64, 0], [48000.0, 0.0])                                # ... is not looked at where n = 0
    assert s.get_emits().tolist() == [0, 0]
