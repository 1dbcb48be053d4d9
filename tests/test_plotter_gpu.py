"""The batch plotter on the device: every view of a PlotterBatch against plotter_ref.RefPlotter, one restated CPlotter per
view, standing on the project's own csdr_fft_batch_get_screen (exact, word for word) and on the fp64 checker's
GetScreenIntegerFFTData (within one count, the bound test_screen_mapping_on_device_for_all_channels holds for fp32 bels).
Shapes are the smallest at which the kernel can go wrong: 512 and 2048 points, views a few hundred pixels wide that hit
both branches of the mapping, its boundary from both sides, w > n, a span wider than the sample rate, 1 to 64 lanes per
pixel, and rings of 3 and 7 lines."""
import ctypes as C

import numpy as np
import pytest

import plotter_ref as R
from util_signals import tones_plus_noise

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def ca():
    import cutesdr_amd
    return cutesdr_amd


def frame(seed, n, fs, rows=2, hot=()):
    """one tones-plus-noise frame per row; rows in `hot` get a sample with re above 32000 (fft.cpp:275)"""
    x = np.stack([tones_plus_noise(seed * 16 + c, n, fs, [0.11 * fs * (c + 1), -0.23 * fs, 0.0371 * fs * (seed % 5)]) for c in range(rows)])
    for c in hot:
        x[c, 5] = 32500.0 + 0j
    return x


def own_screen(ca, b, row):
    """(mapping, overload) of a row through csdr_fft_batch_get_screen, the function that defines what a view shows"""
    flag = []

    def mapping(h, w, max_db, min_db, lo, hi):
        out = np.zeros(max(w, 1), dtype=np.int32)
        rc = ca.lib().csdr_fft_batch_get_screen(b.h, row, h, w, float(max_db), float(min_db), lo, hi, out.ctypes.data_as(C.c_void_p))
        assert rc >= 0
        flag.append(rc)
        return out[:w]
    mapping(1, 1, 0.0, -1.0, 0, 0)
    return mapping, bool(flag[0])


class Pair:
    """a PlotterBatch and one RefPlotter per view, driven by the same calls"""

    def __init__(self, ca, views, rows):
        self.ca, self.p, self.rows = ca, ca.PlotterBatch(views), list(rows)
        self.refs = [R.RefPlotter() for _ in range(views)]
        for v, row in enumerate(rows):
            self.p.set_source(row, v)

    def slot(self, name, *args, view):
        getattr(self.p, name)(*args, view=view)
        getattr(self.refs[view], name)(*args)

    def draw(self, b, mapping_of=None):
        n = self.p.draw(b)
        for v, r in enumerate(self.refs):
            mapping, over = own_screen(self.ca, b, self.rows[v])
            r.draw((mapping_of(v) if mapping_of else None) or mapping, over)
        return n

    def check(self, what, views=None):
        for v in (range(len(self.refs)) if views is None else views):
            r = self.refs[v]
            assert self.p.geometry(v) == r.geometry(), (what, v)
            y, red = self.p.trace(v)
            assert np.array_equal(y, r.trace), (what, v, "trace")
            assert red == r.pen_red, (what, v, "pen")
            assert np.array_equal(self.p.waterfall(v), r.waterfall), (what, v, "waterfall")


def six_views(ca, n, fs):
    """views 0-2 on row 0, 3-4 on row 1, 5 not running; (w, H, percent, span, MaxdB, step) all different"""
    k = int(fs) // 1000                                   # fs = 1000 n: one bin per kHz
    assert k == n
    settings = [
        (20, 200, 50, int(0.9 * fs), 0, 10),              # bins > pixels, 23 (512) / 92 (2048) bins per pixel: 32 / 64 lanes
        (300, 301, 30, 100000, -10, 8),                   # bins < pixels
        (200, 150, 100, 200000, -20, 9),                  # range == w: the pixel branch; no waterfall
        (199, 120, 0, 200000, 0, 7),                      # range == w + 1: the bin branch, 2 lanes; no 2D pixmap, m_MindB stale
        (600, 90, 60, 3 * int(fs), -5, 11),               # span > fs: both bins clamp; w > n at 512 points
        (64, 64, 50, 50000, 0, 10),                       # not running
    ]
    q = Pair(ca, 6, [0, 0, 0, 1, 1, 1])
    for v, (w, H, pct, span, mx, step) in enumerate(settings):
        q.slot("SetPercent2DScreen", pct, view=v)
        q.slot("SetSpanFreq", span, view=v)
        q.slot("SetMaxdB", mx, view=v)
        q.slot("SetdBStepSize", step, view=v)
        q.slot("resizeEvent", w, H, view=v)
        q.slot("SetRunningState", v != 5, view=v)
    return q, settings


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("n", [512, 2048])
def test_views_against_the_projects_own_mapping(ca, n, invert):
    fs = 1000.0 * n
    b = ca.FftBatch(2)
    b.set_params(n, invert, 0.0, fs)
    b.set_ave(1)
    b.put_display(frame(1, n, fs))
    q, settings = six_views(ca, n, fs)
    assert q.refs[3].geometry() == (199, 0, 120, -130) and q.refs[2].geometry()[2] == 0
    # view 5 is drawn once on another frame and on an overloaded row, then stopped: trace, image and pen it holds are real
    # words that the draw below must leave alone
    q.slot("SetRunningState", True, view=5)
    for v in range(5):
        q.slot("SetRunningState", False, view=v)
    b.put_display(frame(3, n, fs, hot=(1,)))
    assert q.draw(b) == 1
    q.slot("SetRunningState", False, view=5)
    for v in range(5):
        q.slot("SetRunningState", True, view=v)
    before = (q.p.trace(5)[0].copy(), q.p.trace(5)[1], q.p.waterfall(5).copy())
    assert before[0].any() and before[1] and (before[2][0] != R.BLACK).any() and (before[2][1:] == R.BLACK).all()
    b.put_display(frame(1, n, fs))
    assert q.draw(b) == 5
    q.check("one draw")
    tbl = R.color_table()
    for v in range(5):
        w, h2d, wf_h, min_db = q.p.geometry(v)
        span, max_db = settings[v][3], settings[v][4]
        mapping, over = own_screen(ca, b, q.rows[v])
        y, red = q.p.trace(v)
        assert np.array_equal(y, mapping(h2d, w, max_db, min_db, R.cdiv(-span, 2), R.cdiv(span, 2))), v
        assert red == over and not red
        img = q.p.waterfall(v)
        assert img.shape == (wf_h, w)
        if wf_h:
            assert np.array_equal(img[0], tbl[255 - mapping(255, w, max_db, min_db, R.cdiv(-span, 2), R.cdiv(span, 2))]), v
            assert (img[1:] == R.BLACK).all(), v
            assert len(set(img[0].tolist())) > 2, v        # the line resolves the spectrum
    after = q.p.trace(5)
    assert np.array_equal(after[0], before[0]) and after[1] == before[1] and np.array_equal(q.p.waterfall(5), before[2])


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("n", [512, 2048])
def test_views_against_the_fp64_checker(ca, oracle, n, invert):
    fs = 1000.0 * n
    x = frame(2, n, fs)
    b = ca.FftBatch(2)
    b.set_params(n, invert, 0.0, fs)
    b.set_ave(1)
    b.put_display(x)
    chk = []
    for c in range(2):
        r = oracle.CFft()
        r.SetFFTParams(n, invert, 0.0, fs)
        r.SetFFTAve(1)
        r.PutInDisplayFFT(x[c])
        chk.append(r)
    q, settings = six_views(ca, n, fs)

    def checker_mapping(v):
        if q.refs[v].w > n:
            return None                                   # the checker's translate table has n entries, as the reference's
        return lambda h, w, mx, mn, lo, hi: chk[q.rows[v]].GetScreenIntegerFFTData(h, w, float(mx), float(mn), lo, hi)[1]
    q.draw(b, mapping_of=checker_mapping)
    tbl = R.color_table()
    for v in range(5):
        w, h2d, wf_h, _ = q.p.geometry(v)
        if w > n:
            continue
        r = q.refs[v]
        y, _ = q.p.trace(v)
        assert np.abs(y.astype(np.int64) - r.trace).max() <= 1, v
        if wf_h:
            span, max_db = settings[v][3], settings[v][4]
            want = chk[q.rows[v]].GetScreenIntegerFFTData(255, w, float(max_db), float(r.m_MindB), R.cdiv(-span, 2), R.cdiv(span, 2))[1]
            line = q.p.waterfall(v)[0]
            near = [tbl[255 - np.clip(want + d, 0, 255)] for d in (-1, 0, 1)]
            assert ((line == near[0]) | (line == near[1]) | (line == near[2])).all(), v
            assert (line == near[1]).mean() > 0.9, v


@pytest.mark.parametrize("invert", [False, True])
def test_stale_min_db_above_max_db(ca, invert):
    """m_MindB only follows at UpdateOverlay, and never in a view without a 2D pixmap, so m_MaxdB can end up BELOW it: the
    gain is positive, the level rises with the bel and csdr_fft_batch_get_screen shows a pixel's WEAKEST bin.  The views
    must do the same, word for word, in the "more bins than pixels" branch with 64, 8 and 2 lanes per pixel."""
    n, fs = 2048, 2048000.0
    b = ca.FftBatch(2)
    b.set_params(n, invert, 0.0, fs)
    b.set_ave(1)
    b.put_display(frame(4, n, fs))
    q = Pair(ca, 4, [0, 1, 1, 0])
    for v, (w, span, pct) in enumerate(((20, 1840000, 50), (300, 1840000, 0), (700, 1400000, 30), (20, 1840000, 50))):
        q.slot("SetSpanFreq", span, view=v)
        q.slot("resizeEvent", w, 400, view=v)
        q.slot("SetMaxdB", 130, view=v)
        q.slot("UpdateOverlay", view=v)                   # m_MindB = -10
        q.slot("SetPercent2DScreen", pct, view=v)         # view 1: no 2D pixmap from here on, m_MindB stays for ever
        q.slot("SetMaxdB", -130 if v < 3 else 130, view=v)    # the first three without UpdateOverlay; view 3 is the upright twin of view 0
        q.slot("UpdateOverlay", view=1)
        q.slot("SetRunningState", True, view=v)
    assert [r.m_MindB for r in q.refs] == [-10] * 4 and [r.m_MaxdB for r in q.refs] == [-130, -130, -130, 130]
    assert q.draw(b) == 4
    q.check("inverted range")
    y0, y3 = q.p.trace(0)[0], q.p.trace(3)[0]
    assert len(set(y0.tolist())) > 3 and y0.max() < 200                  # the inverted views resolve the spectrum
    # the weakest bin of a pixel is never a tone: the upright twin shows the tones, the inverted view must not
    mapping, _ = own_screen(ca, b, 0)
    assert np.array_equal(y0, mapping(200, 20, -130, -10, -920000, 920000))
    assert np.array_equal(y3, mapping(200, 20, 130, -10, -920000, 920000))
    lines = [q.p.waterfall(v)[0] for v in range(3)]
    assert all(len(set(l.tolist())) > 3 for l in lines)


def test_scrolling_and_the_three_readers(ca):
    n, fs = 512, 512000.0
    b = ca.FftBatch(2)
    b.set_params(n, False, 0.0, fs)
    b.set_ave(1)
    q = Pair(ca, 3, [0, 1, 1])
    for v, (w, H, span) in enumerate(((64, 6, 400000), (37, 14, 90000), (0, 30, 300000))):      # rings of 3 and 7 lines, 8 and 4 lanes per pixel; a view without width
        q.slot("SetSpanFreq", span, view=v)
        q.slot("resizeEvent", w, H, view=v)
        q.slot("SetRunningState", True, view=v)
    assert q.refs[0].wf_h == 3 and q.refs[1].wf_h == 7
    stride = 80
    d_lines, d_img = ca.DeviceBuffer(3 * stride * 4), ca.DeviceBuffer(7 * 64 * 4)
    d_y, d_pen = ca.DeviceBuffer(3 * stride * 4), ca.DeviceBuffer(3 * 4)
    for k in range(9):                                    # the rings wrap three times and once
        b.put_display(frame(10 + k, n, fs))
        assert q.draw(b) == 2                             # the view without width runs, takes the pen step, draws nothing
        q.check("draw %d" % k)
        d_lines.upload(np.full(3 * stride, 0x11223344, dtype=np.uint32))
        d_y.upload(np.full(3 * stride, -9, dtype=np.int32))
        q.p.lines_all_ptr(d_lines.ptr, stride)
        q.p.traces_all_ptr(d_y.ptr, stride, d_pen.ptr)
        for v in (0, 1):
            assert q.p.waterfall_ptr(v, d_img.ptr) == q.refs[v].wf_h
            ca.sync()
            w, wf_h = q.refs[v].w, q.refs[v].wf_h
            assert np.array_equal(d_img.download(np.uint32, wf_h * w).reshape(wf_h, w), q.refs[v].waterfall), (k, v)
        ca.sync()
        lines = d_lines.download(np.uint32, 3 * stride).reshape(3, stride)
        ys = d_y.download(np.int32, 3 * stride).reshape(3, stride)
        for v in (0, 1):
            w = q.refs[v].w
            assert np.array_equal(lines[v, :w], q.refs[v].waterfall[0]) and (lines[v, w:] == 0x11223344).all(), (k, v)
            assert np.array_equal(ys[v, :w], q.refs[v].trace) and (ys[v, w:] == -9).all(), (k, v)
        assert (lines[2] == 0x11223344).all() and (ys[2] == -9).all()
        assert not d_pen.download(np.int32, 3).any()
    assert len({q.refs[1].waterfall[r].tobytes() for r in range(7)}) == 7


def test_resize_and_percent_in_mid_stream(ca):
    n, fs = 512, 512000.0
    b = ca.FftBatch(1)
    b.set_params(n, False, 0.0, fs)
    b.set_ave(1)
    q = Pair(ca, 1, [0])
    q.slot("SetSpanFreq", 400000, view=0)
    q.slot("resizeEvent", 90, 10, view=0)
    q.slot("SetRunningState", True, view=0)
    for k in range(4):
        b.put_display(frame(30 + k, n, fs, rows=1))
        q.draw(b)
    q.check("four lines")
    assert (q.p.waterfall(0)[:4] != R.BLACK).any(axis=1).all()
    q.slot("resizeEvent", 90, 10, view=0)                 # the same size: black again
    q.check("blackened")
    assert (q.p.waterfall(0) == R.BLACK).all()
    q.draw(b)
    q.check("one line")
    assert (q.p.waterfall(0)[1:] == R.BLACK).all() and (q.p.waterfall(0)[0] != R.BLACK).any()
    q.draw(b)
    q.slot("SetPercent2DScreen", 20, view=0)
    assert q.p.geometry(0)[:3] == (90, 2, 8)
    q.check("percent")
    assert (q.p.waterfall(0) == R.BLACK).all() and not q.p.trace(0)[0].any()
    q.draw(b)
    q.check("after percent")
    q.slot("resizeEvent", 333, 40, view=0)                # another width: grows the view
    q.check("resized")
    q.draw(b)
    q.check("at the new width")
    mapping, _ = own_screen(ca, b, 0)
    assert np.array_equal(q.p.trace(0)[0], mapping(8, 333, 0, -140, -200000, 200000))


def test_overload_pen(ca):
    n, fs = 512, 512000.0
    b = ca.FftBatch(2)
    b.set_params(n, False, 0.0, fs)
    b.set_ave(1)
    q = Pair(ca, 4, [0, 0, 1, 1])
    for v in range(4):
        q.slot("resizeEvent", 40 + v, 8, view=v)
        q.slot("SetRunningState", True, view=v)
    b.put_display(frame(40, n, fs, hot=(1,)))
    q.draw(b)
    q.check("row 1 overloaded")
    assert [q.p.trace(v)[1] for v in range(4)] == [False, False, True, True]
    b.put_display(frame(41, n, fs))
    q.draw(b)
    q.check("clean again")
    assert not any(q.p.trace(v)[1] for v in range(4))
    q.slot("SetADOverload", True, view=1)
    reds = []
    for k in range(14):
        q.draw(b)
        q.check("one shot %d" % k)
        reds.append([q.p.trace(v)[1] for v in range(4)])
    assert [r[1] for r in reds] == [True] * 12 + [False] * 2
    assert not any(r[0] or r[2] or r[3] for r in reds)
    q.slot("SetADOverload", True, view=0)                 # withdrawn before any draw: the last command counts
    q.slot("SetADOverload", False, view=0)
    q.draw(b)
    q.check("withdrawn")
    assert not q.p.trace(0)[1]


def test_stream_order(ca):
    """put, draw, put, draw enqueued with no host wait in between; then the readers"""
    n, fs = 2048, 2048000.0
    b = ca.FftBatch(1)
    b.set_params(n, False, 0.0, fs)
    b.set_ave(1)
    xs = [np.ascontiguousarray(frame(50 + k, n, fs, rows=1), dtype=np.complex64) for k in range(2)]
    want = []
    for x in xs:                                          # what each spectrum maps to, taken one at a time first
        b.put_display(x)
        mapping, _ = own_screen(ca, b, 0)
        want.append((mapping(10, 150, 0, -140, -900000, 900000), mapping(255, 150, 0, -140, -900000, 900000)))
    assert not np.array_equal(want[0][0], want[1][0])
    p = ca.PlotterBatch(1)
    p.SetSpanFreq(1800000)
    p.resizeEvent(150, 20)
    p.SetRunningState(True)
    bufs = []
    for x in xs:
        d = ca.DeviceBuffer(x.nbytes)
        d.upload(x)
        bufs.append(d)
    ca.sync()
    for d in bufs:
        b.put_display_ptr(d.ptr, n, 1)
        assert p.draw(b) == 1
    y, _ = p.trace(0)
    img = p.waterfall(0)
    tbl = R.color_table()
    assert np.array_equal(y, want[1][0])
    assert np.array_equal(img[0], tbl[255 - want[1][1]]) and np.array_equal(img[1], tbl[255 - want[0][1]])
    assert (img[2:] == R.BLACK).all()
    ca.sync()


def test_refusals_change_nothing(ca):
    n, fs = 512, 512000.0
    b = ca.FftBatch(2)
    b.set_params(n, False, 0.0, fs)
    b.set_ave(1)
    b.put_display(frame(60, n, fs))
    L = ca.lib()

    def make():
        p = ca.PlotterBatch(2)
        p.SetSpanFreq(300000)
        p.resizeEvent(70, 12)
        p.SetRunningState(True)
        return p
    p, clean = make(), make()
    assert not L.csdr_plotter_batch_create(0, 0) and not L.csdr_plotter_batch_create(0, 4097)
    for rc in (L.csdr_plotter_batch_resize(p.h, 0, 4097, 10), L.csdr_plotter_batch_resize(p.h, 0, 10, 4097),
               L.csdr_plotter_batch_resize(p.h, 0, -1, 10), L.csdr_plotter_batch_resize(p.h, -1, 10, -1),
               L.csdr_plotter_batch_resize(p.h, 2, 10, 10), L.csdr_plotter_batch_set_percent_2d(p.h, 0, 101),
               L.csdr_plotter_batch_set_percent_2d(p.h, -1, -1), L.csdr_plotter_batch_set_db_step(p.h, 0, 0),
               L.csdr_plotter_batch_set_span(p.h, 2, 1000), L.csdr_plotter_batch_set_max_db(p.h, 5, 0),
               L.csdr_plotter_batch_set_source(p.h, 0, -1), L.csdr_plotter_batch_set_source(p.h, 2, 0),
               L.csdr_plotter_batch_set_running(p.h, 2, 1), L.csdr_plotter_batch_set_ad_overload(p.h, 2, 1),
               L.csdr_plotter_batch_update_overlay(p.h, 2), L.csdr_plotter_batch_draw(p.h, None, None),
               L.csdr_plotter_batch_get_geometry(p.h, 2, None, None, None, None),
               L.csdr_plotter_batch_get_trace(p.h, -1, None, None)):
        assert rc == EINVAL
    p.set_source(2, 1)                                    # accepted: a row is judged against the spectra at the draw
    assert L.csdr_plotter_batch_draw(p.h, b.h, None) == EINVAL
    assert (p.waterfall(1) == R.BLACK).all() and not p.trace(1)[0].any()       # the refused draw drew nothing
    p.set_source(1, 1)
    d = ca.DeviceBuffer(2 * 64 * 4)
    assert L.csdr_plotter_batch_get_lines_all(p.h, C.c_void_p(d.ptr), 69, None) == EINVAL      # narrower than the views
    assert p.draw(b) == 2 and clean.draw(b) == 2
    for v in range(2):
        assert p.geometry(v) == clean.geometry(v) == (70, 6, 6, -140)
        assert np.array_equal(p.trace(v)[0], clean.trace(v)[0]) and p.trace(v)[0].any()
        assert np.array_equal(p.waterfall(v), clean.waterfall(v))
        assert (p.waterfall(v)[1:] == R.BLACK).all()
