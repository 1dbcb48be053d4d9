"""A plain restatement of one CPlotter's display state and of draw() (reference gui/plotter.cpp: constructor :100-114,
resizeEvent :374-389, draw :408-480, DrawOverlay's m_MindB :597; setters gui/plotter.h:32-44), and of the screen mapping
CFft::GetScreenIntegerFFTData (dsp/fft.cpp:308-410) with this project's two bound fixes, in the operation order of
csdr_fft_batch_get_screen.  Loops as the reference writes them; nothing here is shared with the product."""
import numpy as np

VERT_DIVS = 14
OVERLOAD_DISPLAY_LIMIT = 10
BLACK = 0xFF000000


def cdiv(a, b):
    """C's integer division: truncation towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def color_table():
    """m_ColorTbl (gui/plotter.cpp:67-83) as 0xFFRRGGBB"""
    tbl = []
    for i in range(256):
        r = g = b = 0
        if i < 43:
            b = 255 * i // 43
        elif i < 87:
            g, b = 255 * (i - 43) // 43, 255
        elif i < 120:
            g, b = 255, 255 - (255 * (i - 87) // 32)
        elif i < 154:
            r, g = 255 * (i - 120) // 33, 255
        elif i < 217:
            r, g = 255, 255 - (255 * (i - 154) // 62)
        else:
            r, b = 255, 128 * (i - 217) // 38
        tbl.append(0xFF000000 | ((r & 255) << 16) | ((g & 255) << 8) | (b & 255))
    return np.array(tbl, dtype=np.uint32)


def bin_range(n, fs, start_hz, stop_hz):
    """m_BinMin, m_BinMax (fft.cpp:333-345)"""
    maxbin = n - 1
    bin_min = int(float(start_hz) * float(n) / fs) + n // 2
    bin_max = int(float(stop_hz) * float(n) / fs) + n // 2
    bin_min = max(bin_min, 0)
    if bin_min >= maxbin:
        bin_min = maxbin
    bin_max = max(bin_max, 0)
    if bin_max >= maxbin:
        bin_max = maxbin
    return bin_min, bin_max


def screen(ave, n, invert, fs, max_h, max_w, max_db, min_db, start_hz, stop_hz, runs=None):
    """GetScreenIntegerFFTData on the bels `ave` (display order, any float type: each value goes through a double as the
    reference's does).  runs: a list that receives, per pixel, the bels of the bins that reached it."""
    ave = np.asarray(ave)
    out = [None] * max_w
    if runs is not None:
        runs[:] = [[] for _ in range(max_w)]
    off, gain = max_db / 10.0, -10.0 / (max_db - min_db)
    bin_min, bin_max = bin_range(n, fs, start_hz, stop_hz)
    xlat = [0] * n
    if bin_max - bin_min > max_w:
        for i in range(bin_min, bin_max + 1):
            xlat[i] = ((i - bin_min) * max_w) // (bin_max - bin_min)
    else:
        for i in range(min(max_w, n)):
            xlat[i] = bin_min + (i * (bin_max - bin_min)) // max_w

    def level(b_in):
        b = n - b_in if invert else b_in
        if b >= n:
            b = n - 1                                    # the reference reads one past the end here
        v = int(float(max_h) * gain * (float(ave[b]) - off))
        return min(max(v, 0), max_h), ave[b]

    if bin_max - bin_min > max_w:
        xprev, ymax = -1, 10000
        for i in range(bin_min, bin_max + 1):
            y, a = level(i)
            x = xlat[i]
            if x >= max_w:
                continue                                 # the reference writes OutBuf[MaxWidth] here
            if runs is not None:
                runs[x].append(a)
            if x == xprev:
                if y < ymax:
                    out[x] = y
                    ymax = y
            else:
                out[x] = y
                xprev = x
                ymax = y
    else:
        for x in range(max_w):
            out[x], a = level(xlat[x if x < n else n - 1])
            if runs is not None:
                runs[x].append(a)
    assert all(v is not None for v in out), "a pixel no bin reached"
    return np.array(out, dtype=np.int32)


class RefPlotter:
    """One CPlotter.  mapping(max_h, max_w, max_db, min_db, start_hz, stop_hz) -> levels [max_w] stands for
    m_pSdrInterface->GetScreenIntegerFFTData, `overload` for its return value."""

    def __init__(self):
        self.m_Span, self.m_MaxdB, self.m_MindB, self.m_dBStepSize = 50000, 0, -130, 10     # :100-103
        self.m_Running = False
        self.m_ADOverloadOneShotCounter, self.m_ADOverLoad = 0, False
        self.m_Percent2DScreen = 50
        self.size = self.m_Size = (0, 0)                 # the widget's size; what the last resize event saw
        self.w, self.h2d, self.wf_h = 0, 0, 0
        self.waterfall = np.zeros((0, 0), dtype=np.uint32)
        self.trace = np.zeros(0, dtype=np.int32)
        self.pen_red = False
        self.tbl = color_table()

    def resizeEvent(self, w, h):
        changed = self.m_Size != (w, h)                                           # :378
        self.size = self.m_Size = (w, h)
        self.w = w
        self.h2d = self.m_Percent2DScreen * h // 100
        if changed:
            self.trace = np.zeros(self.w, dtype=np.int32)                         # a new, black m_2DPixmap: no trace yet
        self.wf_h = (100 - self.m_Percent2DScreen) * h // 100
        self.waterfall = np.full((self.wf_h, self.w), BLACK, dtype=np.uint32)     # fill(Qt::black), on every event :387
        self.DrawOverlay()

    def SetPercent2DScreen(self, percent):
        self.m_Percent2DScreen = percent
        self.m_Size = (0, 0)                                                      # plotter.h:35
        self.resizeEvent(*self.size)

    def SetSpanFreq(self, s):
        self.m_Span = s

    def SetMaxdB(self, v):
        self.m_MaxdB = v

    def SetdBStepSize(self, v):
        self.m_dBStepSize = v

    def DrawOverlay(self):
        if self.w == 0 or self.h2d == 0:
            return                                       # m_OverlayPixmap.isNull()
        self.m_MindB = self.m_MaxdB - VERT_DIVS * self.m_dBStepSize                 # :597

    UpdateOverlay = DrawOverlay

    def SetADOverload(self, on):
        self.m_ADOverLoad = bool(on)
        self.m_ADOverloadOneShotCounter = 0

    def SetRunningState(self, running):
        self.m_Running = bool(running)

    def geometry(self):
        return self.w, self.h2d, self.wf_h, self.m_MindB

    def draw(self, mapping, overload):
        if not self.m_Running:
            return
        lo, hi = cdiv(-self.m_Span, 2), cdiv(self.m_Span, 2)
        if self.wf_h > 0 and self.w > 0:
            self.waterfall[1:] = self.waterfall[:-1].copy()                         # scroll(0, 1, ...) :425
            line = mapping(255, self.w, self.m_MaxdB, self.m_MindB, lo, hi)
            self.waterfall[0] = self.tbl[255 - np.asarray(line)]                    # :436-441
        if self.w > 0:
            self.trace = np.asarray(mapping(self.h2d, self.w, self.m_MaxdB, self.m_MindB, lo, hi), dtype=np.int32)
        if self.m_ADOverLoad or overload:                                           # :458-468
            self.pen_red = True
            c = self.m_ADOverloadOneShotCounter
            self.m_ADOverloadOneShotCounter += 1
            if c > OVERLOAD_DISPLAY_LIMIT:
                self.m_ADOverloadOneShotCounter = 0
                self.m_ADOverLoad = False
        else:
            self.pen_red = False
