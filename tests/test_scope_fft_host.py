"""CPU checks of the batch scope's FFT view: the host-side pieces of cutesdr_amd/csrc/scope_host.hpp, through the
csdr__host_scope_fft_* hooks (the functions capi_scope.hip and scope_kernels.hip evaluate), against scope_fft_ref.py,
the restatement of the reference's frequency branch (gui/testbench.cpp:594-611, :654-672, :1005-1068), and against
the fp64 oracle's CFft.  All comparisons are on integers or words and exact."""
import ctypes as C

import numpy as np
import pytest

import scope_fft_ref as F
import scope_ref as R

SYMBOLS = ["csdr_scope_batch_" + s for s in (
    "set_time_display", "enable_peak", "get_fft_screen", "get_fft_ave", "get_fft_state", "get_fft_screens_all")]


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_scope_fft_plan.restype = None
    lib.csdr__host_scope_fft_plan.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p]
    lib.csdr__host_scope_fft_settings.restype = None
    lib.csdr__host_scope_fft_settings.argtypes = [C.c_int, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.csdr__host_scope_fft_chan.restype = None
    lib.csdr__host_scope_fft_chan.argtypes = [C.c_void_p, C.c_void_p]
    lib.csdr__host_scope_fft_frame.restype = None
    lib.csdr__host_scope_fft_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_longlong, C.c_void_p]
    lib.csdr__host_scope_fft_map.restype = None
    lib.csdr__host_scope_fft_map.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.csdr__host_scope_create.restype = C.c_void_p
    lib.csdr__host_scope_destroy.argtypes = [C.c_void_p]
    lib.csdr__host_scope_slot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.csdr__host_scope_put.restype = C.c_longlong
    lib.csdr__host_scope_put.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double]
    return lib


def test_symbols_exported_and_bound(L):
    from cutesdr_amd import _capi
    names = _capi.declared_symbols()
    for s in SYMBOLS:
        assert s in names, s
        assert getattr(L, s).argtypes is not None, s
    import cutesdr_amd
    for slot in ("OnTimeDisplay", "OnEnablePeak", "get_fft_screen", "get_fft_ave", "get_fft_state", "get_fft_screens_all"):
        assert hasattr(cutesdr_amd.ScopeBatch, slot), slot


def literal_loop(pos, cnt, skip, n):
    """gui/testbench.cpp:597-610 without the data: the completing frames that are used"""
    used, frames = [], 0
    for _ in range(n):
        pos += 1
        if pos >= F.TEST_FFTSIZE:
            pos = 0
            cnt += 1
            if cnt >= skip:
                cnt = 0
                used.append(frames)
            frames += 1
    return frames, used, pos, cnt


def test_planner_equals_the_literal_loop(L):
    """random position, counter in -2 .. skip and n; skip values 0, 1, 3, 97 and one larger than the call's frames"""
    rng = np.random.default_rng(11)
    out = np.zeros(6, dtype=np.int64)
    some = 0
    for skip in (0, 1, 3, 97, 5000):
        for _ in range(60):
            pos = int(rng.integers(0, F.TEST_FFTSIZE))
            cnt = int(rng.integers(-2, skip + 1))
            n = int(rng.choice([0, 1, 7, 2047, 2048, 2049, 5000, int(rng.integers(1, 250000))]))
            frames, used, pos_end, cnt_end = literal_loop(pos, cnt, skip, n)
            L.csdr__host_scope_fft_plan(pos, cnt, skip, n, out.ctypes.data)
            fr, first, step, count, pe, ce = out.tolist()
            assert (fr, count, pe, ce) == (frames, len(used), pos_end, cnt_end), (skip, pos, cnt, n)
            assert [first + k * step for k in range(count)] == used, (skip, pos, cnt, n)
            some += count
    assert some > 500                                    # not vacuous: hundreds of used frames were compared
    frames, used, _, _ = literal_loop(0, -2, 5000, 40 * 2048)                   # larger than the call's frames: none
    assert frames == 40 and used == []


def test_settings(L):
    skip, span = C.c_int(), C.c_int()
    for sr, rate, want in ((62500.0, 10, 3), (2.0e6, 10, 97)):
        L.csdr__host_scope_fft_settings(rate, sr, C.byref(skip), C.byref(span))
        assert skip.value == want == R.c_int(sr / (2048 * rate))
    for sr, want in ((48000.0, 48000), (48001.0, 48000), (12345.0, 12350), (62500.0, 62500), (1.0, 0), (7.0, 10), (2147483631.0, 2147483630)):
        L.csdr__host_scope_fft_settings(10, sr, C.byref(skip), C.byref(span))
        s = R.c_int(sr)
        assert span.value == want == s - F.c_rem(s + 5, 10) + 5, sr


def chan(L, h):
    out = np.zeros(8, dtype=np.int64)
    L.csdr__host_scope_fft_chan(h, out.ctypes.data)
    return dict(zip(("view", "skip", "span", "pos", "cnt", "cur", "flags", "peak_on"), out.tolist()))


def test_skip_value_follows_the_view(L, oracle):
    """OnTimeDisplay is a Reset that computes the skip value of the new view; OnDisplayRate computes the view's own;
    OnHorzSpan in the FFT view only stores the span; the host's position and counter equal the restatement's"""
    h = L.csdr__host_scope_create()
    r = F.RefFftScope(oracle)
    sr = 62500.0
    x = np.zeros(9000, dtype=np.float32)

    def both(what, v):
        L.csdr__host_scope_slot(h, what, v, 0)
        {1: r.OnHorzSpan, 2: r.OnDisplayRate, 8: r.OnTimeDisplay, 9: r.OnEnablePeak}[what](v)

    def put(n):
        L.csdr__host_scope_put(h, x.ctypes.data, None, n, sr)
        r.DisplayData(x[:n].tolist(), None, sr)
        k = chan(L, h)
        assert k["skip"] == r.m_DisplaySkipValue and k["view"] == (0 if r.m_TimeDisplay else 1)
        if not r.m_TimeDisplay:
            assert (k["pos"], k["cnt"], k["span"]) == (r.m_FftBufPos, r.m_DisplaySkipCounter, r.m_Span)

    put(100)                                             # the first call: a new rate, dropped
    assert chan(L, h)["skip"] == 1 == r.m_DisplaySkipValue                      # time view: 62500 / (6250 * 10)
    both(8, 0); put(5000)
    assert chan(L, h)["skip"] == 3 and chan(L, h)["pos"] == 5000 - 4096
    both(1, 7)                                           # the span alone: the skip value stays
    assert chan(L, h)["skip"] == 3 == r.m_DisplaySkipValue
    both(2, 1); put(9000)
    assert chan(L, h)["skip"] == 30
    both(8, 1)
    assert chan(L, h)["skip"] == r.m_DisplaySkipValue == R.c_int(sr / ((7 * sr / 1000.0) * 1))
    both(8, 0)
    assert chan(L, h)["skip"] == 30 and chan(L, h)["pos"] == 0 and chan(L, h)["cnt"] == -2
    both(9, 1)
    assert chan(L, h)["flags"] & 4 and chan(L, h)["peak_on"] == 1
    put(2049)
    assert chan(L, h)["flags"] == 0
    L.csdr__host_scope_destroy(h)


@pytest.mark.parametrize("cpx", [False, True], ids=["real", "complex"])
def test_frame_assembly_equals_restatement(L, oracle, cpx):
    """over uneven cuts the samples the kernel's frame load picks for every used frame are, word for word, the
    m_FftInBuf the restatement hands to PutInDisplayFFT"""
    sr, n_total = 62500.0, 30 * 2048 + 77
    x = F.feed_signal(0, n_total, sr, cpx)
    seen = []

    class Spy(F.RefFftScope):
        def DrawFftPlot(self):
            seen.append(self.m_FftInBuf.astype(np.complex64))

    r = Spy(oracle)
    r.OnTimeDisplay(False)
    r.DisplayData([], [] if cpx else None, sr)           # the new rate
    rng = np.random.default_rng(3)
    carry, fill, cnt, pos = np.zeros(2048, dtype=np.complex64), 0, -2, 0
    out6, frame = np.zeros(6, dtype=np.int64), np.zeros(2048, dtype=np.complex64)
    got = []
    while pos < n_total:
        n = min(int(rng.choice([1, 7, 256, 513, 2048, 2049, 5000])), n_total - pos)
        row = np.ascontiguousarray(x[pos:pos + n])
        r.DisplayData(row.real.tolist(), row.imag.tolist() if cpx else None, sr)
        L.csdr__host_scope_fft_plan(fill, cnt, r.m_DisplaySkipValue, n, out6.ctypes.data)
        frames, first, step, count, pos_end, cnt_end = out6.tolist()
        for k in range(count):
            L.csdr__host_scope_fft_frame(carry.ctypes.data, fill, row.ctypes.data, int(cpx), first + k * step, frame.ctypes.data)
            got.append(frame.copy())
        rc = row.astype(np.complex64)
        if frames == 0:                                  # the put's carry handling, as scope_put_kernel's
            carry[fill:fill + n] = rc
        else:
            carry[:pos_end] = rc[n - pos_end:]
        fill, cnt, pos = pos_end, cnt_end, pos + n
        assert (fill, cnt) == (r.m_FftBufPos, r.m_DisplaySkipCounter)
    assert len(got) == len(seen) >= 7
    for a, b in zip(got, seen):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("cpx,w", [(True, 100), (True, 700), (True, 2047), (True, 2048), (False, 500), (False, 1500)])
@pytest.mark.parametrize("h", [100, 255])
def test_mapping_equals_the_oracle(L, oracle, cpx, w, h):
    """fed the oracle's bels the mapping hook equals GetScreenIntegerFFTData exactly, in both branches; so do the
    restatement's own lines (scope_fft_ref.map_lines), which the GPU test runs on bels +- tol"""
    sr = 48001.0
    r = F.RefFftScope(oracle)
    r.resizeEvent(w, h)
    r.OnTimeDisplay(False)
    r.OnDisplayRate(100)                                 # a skip value of 0: of three frames the last two are drawn
    x = F.feed_signal(1, 3 * 2048, sr, cpx)
    r.DisplayData([], [] if cpx else None, sr)
    r.DisplayData(x.real.tolist(), x.imag.tolist() if cpx else None, sr)
    assert len(r.draws) == 2 and r.m_Span == 48000
    F.assert_above_floor(r.draws)
    out, m4 = np.zeros(w, dtype=np.int32), np.zeros(4, dtype=np.int32)
    branches = set()
    for d in r.draws:
        bels = np.ascontiguousarray(d.bels)
        L.csdr__host_scope_fft_map(r.m_Span, int(cpx), sr, w, h, bels.ctypes.data, out.ctypes.data, m4.ctypes.data)
        assert out.tolist() == d.y
        assert F.map_lines(d.bels, d.fs, h, w, d.start, d.stop) == d.y
        assert 0 < min(d.y) < max(d.y) <= h
        branches.add(int(m4[2]))
        assert m4[3] == h and (m4[1] - m4[0] > w) == bool(m4[2])
    assert branches == ({1} if w < (2047 if cpx else 1023) else {0})
