"""The display spectrum on the device (K3: spectrum_kernels.hip, fft_generic_kernels.hip, and the scope's FFT view) held
to the rule of k3_bins.py: per row E <= m E_y -- E the largest error of one bin's amplitude against the fp64 oracle fed
frame by frame, over the rms bin amplitude; E_y the same figure of an fp32 restatement of the pipeline on the CPU;
m = 4 (6.43 at 16384 points) -- on flat-spectrum probes, a distinct one per frame and row.

Each of the eight sizes is a configuration of its own (512, 1024, 32768, 65536: the multi-launch form; 2048, 4096, 8192:
sixteen points per thread, a pass B each; 16384: thirty-two per thread), so every test runs all eight.  Every test
prints E / E_y.

The overload flag is the last put frame's (fft.cpp:270 clears it at the top of every PutInDisplayFFT): exact against the
oracle, for hot samples in every part of the frame that another thread or slot loads, the strict `>`, the imaginary
part, a negative real part and a hot sample in an earlier frame of the call."""
import ctypes as C

import numpy as np
import pytest

import k3_bins as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ca():
    import torch                                         # before the library, as everywhere in this suite (the scope test uses it)
    import cutesdr_amd
    torch.cuda.init()
    return cutesdr_amd


def batch(ca, channels, n, ave):
    fb = ca.FftBatch(channels)
    fb.set_params(n, False, 0.0, K.FS)
    fb.set_ave(ave)
    return fb


def check_rows(fb, refs, yards, n, what):
    worst = 0.0
    for c, (r, y) in enumerate(zip(refs, yards)):
        ref = r.ave_buf()
        e_y = K.figure(y.ave_buf(), ref, n)
        worst = max(worst, K.check(fb.ave_buf(c), ref, e_y, n, "%s row %d" % (what, c)))
    print("%s n=%d: worst E / E_y = %.2f (m = %g)" % (what, n, worst, K.margin(n)))
    return worst


def pairs(oracle, n, rows, ave):
    return [K.oracle_fft(oracle, n, ave) for _ in range(rows)], [K.Yard32(n, ave) for _ in range(rows)]


def put(fb, refs, yards, x):
    """x [rows, nframes, n]: one put_display call, and the same frames into the references"""
    fb.put_display(x.reshape(x.shape[0], -1))
    for c in range(x.shape[0]):
        K.feed((refs[c], yards[c]), x[c])


# 1 ---- transform, scatter and log alone
@pytest.mark.parametrize("n", K.SIZES)
def test_one_frame_no_average(ca, oracle, n):
    fb = batch(ca, 3, n, 1)
    refs, yards = pairs(oracle, n, 3, 1)
    put(fb, refs, yards, K.frames(n, 3, 1, case=10))
    check_rows(fb, refs, yards, n, "one frame")
    assert [fb.total_count(c) for c in range(3)] == [1, 1, 1]


# 2 ---- the warm-up ends inside the second call, the exponential phase follows
@pytest.mark.parametrize("n", K.SIZES)
def test_average_across_two_calls(ca, oracle, n):
    fb = batch(ca, 2, n, 3)
    refs, yards = pairs(oracle, n, 2, 3)
    put(fb, refs, yards, K.frames(n, 2, 2, case=11))
    check_rows(fb, refs, yards, n, "ave 3, after 2 frames")
    put(fb, refs, yards, K.frames(n, 2, 5, case=11, first=2))
    check_rows(fb, refs, yards, n, "ave 3, after 2 + 5 frames")
    assert [fb.total_count(c) for c in range(2)] == [7, 7]


# 3 ---- frame groups: spectrum_alpha_kernel and spectrum_combine_kernel, a reset, a count above the new size
@pytest.mark.parametrize("n", K.SIZES)
def test_frame_groups(ca, oracle, n):
    fb = batch(ca, 1, n, 4)
    refs, yards = pairs(oracle, n, 1, 4)
    for call in range(2):                                # 16 frames: nparts = 16 / 8 = 2
        put(fb, refs, yards, K.frames(n, 1, 16, case=12, first=16 * call))
        check_rows(fb, refs, yards, n, "groups, call %d" % call)
        assert fb.total_count(0) == 16 * (call + 1)
    fb.set_ave(2)
    for o in refs + yards:
        o.SetFFTAve(2)
    put(fb, refs, yards, K.frames(n, 1, 16, case=12, first=32))
    check_rows(fb, refs, yards, n, "groups, after set_ave(2)")
    assert fb.total_count(0) == 16                       # (SetFFTAve resets, fft.cpp:103-113)


# 4 ---- the one-object form
@pytest.mark.parametrize("n", K.SIZES)
def test_one_object_put_in_display_fft(ca, oracle, n):
    f = ca.CFft()
    f.SetFFTParams(n, False, 0.0, K.FS)
    f.SetFFTAve(2)
    r, y = K.oracle_fft(oracle, n, 2), K.Yard32(n, 2)
    for k, fr in enumerate(K.frames(n, 1, 3, case=13)[0]):
        wide = fr.astype(np.complex128)
        assert f.PutInDisplayFFT(wide) == r.PutInDisplayFFT(wide) == y.PutInDisplayFFT(wide) == k + 1
    ref = r.ave_buf()
    K.check(f.ave_buf(), ref, K.figure(y.ave_buf(), ref, n), n, "CFft, ave 2, 3 frames")


# 5 ---- the scope's FFT view
def test_scope_fft_view(ca, oracle):
    """one receiver, whole frames (the carry stays empty), every frame after the first drawn: get_fft_ave is the last
    frame's spectrum without averaging (testbench.cpp:132)"""
    import torch
    n, fs = 2048, 204800.0
    s = ca.ScopeBatch(1)
    s.resizeEvent(700, 255); s.OnTimeDisplay(False); s.OnDisplayRate(1000)          # skip value 0
    x = K.frames(n, 1, 4, case=14)
    rows = torch.from_numpy(x.reshape(1, -1).copy()).cuda()
    s.DisplayData(rows, 1, fs)                           # the call that brings the new rate is dropped
    for call, (first, count) in enumerate(((0, 1), (1, 1), (2, 2))):
        s.DisplayData(rows, count * n, fs, offset=first * n)
        last = first + count - 1
        state = s.get_fft_state(0).tolist()
        assert state[0] == 0, state                      # nothing carried
        if last == 0:
            assert state[3] == 0                         # the first complete frame after a reset is never used
            continue
        assert state[3] == last
        ref, e_y = K.reference(oracle, x[0, last:last + 1], 1)
        K.check(s.get_fft_ave(0), ref, e_y, n, "scope FFT view, call %d" % call)


# 6 ---- overload
HOT = np.nextafter(np.float32(K.OVER_LIMIT), np.float32(np.inf))


def hot_positions(n):
    """0, 1, n/2, n-1 and one place in each of eight further sixteenths of the frame"""
    s = n // 16
    return [0, 1, n // 2, n - 1] + [k * s + (5 + 7 * k) % s for k in (1, 2, 3, 5, 6, 10, 12, 14)]


def overload_rows(n):
    """(x [16, 2, n], expected flags): 12 rows hot in the last frame, then re == limit, im hot, re = -32700, frame 0 only"""
    x = K.frames(n, 16, 2, case=15).copy()
    assert np.abs(x.real).max() < 12000 and np.abs(x.imag).max() < 12000
    pos = hot_positions(n)
    assert len(set(pos)) == 12 and len({p // (n // 16) for p in pos}) == 11 and all(0 <= p < n for p in pos)
    for r, p in enumerate(pos):
        x[r, 1, p] = HOT + 1j * x[r, 1, p].imag
    x[12, 1, 5] = np.float32(K.OVER_LIMIT) + 1j * x[12, 1, 5].imag
    x[13, 1, 5] = x[13, 1, 5].real + 32700j
    x[14, 1, 5] = -32700.0 + 1j * x[14, 1, 5].imag
    x[15, 0, 5] = HOT + 1j * x[15, 0, 5].imag
    assert x.dtype == np.complex64 and x[0, 1, 0].real > K.OVER_LIMIT and x[12, 1, 5].real == K.OVER_LIMIT
    return x, [True] * 12 + [False] * 4


def oracle_flags(oracle, x, n):
    out = []
    for row in x:
        r = K.oracle_fft(oracle, n, 1)
        K.feed((r,), row)
        out.append(r.GetScreenIntegerFFTData(100, 50, 0.0, -100.0, -1000, 1000)[0])
    return out


def flags_of(ca, fb):
    """the flags through screen_all and through csdr_fft_batch_get_screen"""
    ov, _ = fb.screen_all(100, 50, 0.0, -100.0, -1000, 1000)
    one = np.zeros(51, dtype=np.int32)
    each = [ca.lib().csdr_fft_batch_get_screen(fb.h, c, 100, 50, C.c_double(0.0), C.c_double(-100.0), -1000, 1000,
                                               one.ctypes.data_as(C.c_void_p)) for c in range(fb.channels)]
    assert all(v in (0, 1) for v in each), each
    return [bool(v) for v in ov], [bool(v) for v in each]


@pytest.mark.parametrize("n", K.SIZES)
def test_overload_flag_is_the_last_frames(ca, oracle, n):
    x, want = overload_rows(n)
    assert oracle_flags(oracle, x, n) == want
    fb = batch(ca, 16, n, 1)
    fb.put_display(x.reshape(16, -1))
    all_, each = flags_of(ca, fb)
    assert all_ == want, (n, all_)
    assert each == want, (n, each)
    fb.put_display(x[:, 0].reshape(16, -1))              # frame 0 alone: only the last row is hot now
    all_, each = flags_of(ca, fb)
    assert all_ == each == [False] * 15 + [True]


@pytest.mark.parametrize("n", K.SIZES)
def test_overload_flag_across_frame_groups(ca, oracle, n):
    """16 frames in one call are two frame groups (nparts = 2): only a hot sample in frame 15 counts -- not one in the
    last frame of group 0, nor one in the first frame of group 1"""
    x = K.frames(n, 3, 16, case=17).copy()
    for row, frame in enumerate((7, 15, 8)):
        x[row, frame, n // 3] = HOT + 1j * x[row, frame, n // 3].imag
    want = [False, True, False]
    assert oracle_flags(oracle, x, n) == want
    fb = batch(ca, 3, n, 1)
    fb.put_display(x.reshape(3, -1))
    all_, each = flags_of(ca, fb)
    assert all_ == each == want, (n, all_, each)


@pytest.mark.parametrize("carry", [0, 100])
def test_overload_flag_through_the_stream(ca, oracle, carry):
    """two used frames in one put_display_stream call at 4096 points, the hot sample in the first of them only -- as one
    launch on the rows in place (carry 0), and as two launches, the first frame begun in the carry"""
    n = 4096
    x = K.frames(n, 2, 3, case=16).reshape(2, -1).copy()
    x[1, carry + 5] = HOT + 1j * x[1, carry + 5].imag    # frame 0 of the frames the second call completes
    fb = batch(ca, 2, n, 1)
    if carry:
        assert fb.put_display_stream(x[:, :carry]) == 0
    assert fb.put_display_stream(x[:, carry:carry + 2 * n]) == 2
    want = oracle_flags(oracle, x[:, :2 * n].reshape(2, 2, n), n)
    assert want == [False, False]
    all_, each = flags_of(ca, fb)
    assert all_ == each == want
    for c in range(2):                                   # ... and the spectrum is the second frame's
        ref, e_y = K.reference(oracle, x[c, n:2 * n][None, :], 1)
        K.check(fb.ave_buf(c), ref, e_y, n, "stream row %d" % c)
