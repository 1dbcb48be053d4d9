"""GPU checks of the display stream (csdr_fft_batch_put_display_stream / _packets, csdr_ingest_spurcal_packets): the
display path of CSdrInterface::ProcessIQData (reference interface/sdrinterface.cpp:878-907) rebuilt in the test from
the oracle's unpack, NcoSpurCalibrate and CFft::PutInDisplayFFT with frame carry, skip counter and screen gate, against
the device on datagram feeds; word equality against the unpack + fp32 forms; independence of how a stream is cut into
calls; bit-equal spur calibration on datagrams; the screen mapping after a datagram feed."""
import ctypes as C
import numpy as np
import pytest
from test_fft_resampler_gpu import assert_spectrum_close
from util_signals import FULL_SCALE

pytestmark = pytest.mark.gpu


def make_packets(x, pkt_len, seq0=0):
    """complex samples on the 16-bit scale [channels, n] -> uint8 datagrams [channels, n / per, pkt_len]
    (interface/netiobase.cpp:479-527: 4 header bytes, little-endian I,Q; 24 bit = 256 x the 16-bit scale)"""
    per = 240 if pkt_len == 1444 else 256
    ch, n = x.shape
    assert n % per == 0
    npk = n // per
    out = np.zeros((ch, npk, pkt_len), dtype=np.uint8)
    out[:, :, 0] = 0x04; out[:, :, 1] = 0x84 if pkt_len == 1444 else 0x04
    out[:, :, 2] = (np.arange(npk) + seq0) & 0xff
    if pkt_len == 1028:
        iq = np.empty((ch, n, 2), dtype=np.int16)
        iq[..., 0] = np.clip(np.round(x.real), -32768, 32767); iq[..., 1] = np.clip(np.round(x.imag), -32768, 32767)
        out[:, :, 4:] = iq.reshape(ch, npk, per * 2).view(np.uint8)
    else:
        v = np.empty((ch, n, 2), dtype=np.int64)
        v[..., 0] = np.clip(np.round(x.real * 256), -(1 << 23), (1 << 23) - 1)
        v[..., 1] = np.clip(np.round(x.imag * 256), -(1 << 23), (1 << 23) - 1)
        u = (v & 0xffffff).astype(np.uint32)
        b = np.stack([u & 0xff, (u >> 8) & 0xff, (u >> 16) & 0xff], axis=-1).astype(np.uint8)   # [ch, n, 2, 3]
        out[:, :, 4:] = b.reshape(ch, npk, per * 6)
    return out


def feed_signal(ch, n, fs, seed, dc=(150.0, -90.0), spike_channel=None):
    """tones at -20 dBFS + noise at -66 dBFS + a DC offset, on the 16-bit scale"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.empty((ch, n), dtype=np.complex128)
    amp, sig = FULL_SCALE * 0.1, FULL_SCALE * 10 ** (-66 / 20.0)
    for c in range(ch):
        f1 = fs * (0.11 + 0.07 * c)
        x[c] = amp * np.exp(2j * np.pi * f1 * t / fs) + 0.3 * amp * np.exp(-2j * np.pi * 0.31 * t) \
            + sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + (dc[0] + 1j * dc[1]) * (1 + 0.2 * c)
    if spike_channel is not None:
        x[spike_channel, n // 3] = 32700.0 + 0j                 # > OVER_LIMIT (fft.cpp:23) after the DC correction
    return x


class OracleDisplay:
    """ProcessIQData's display half for one channel: NcoSpurCalibrate, DC correction into m_DataBuf, skip counter,
    m_ScreenUpateFinished gate, CFft::PutInDisplayFFT (all fp64, the oracle's)."""

    def __init__(self, orc, N, ave, fs, skip, gated):
        self.orc, self.N, self.skip, self.gated = orc, N, skip, gated
        self.fft = orc.CFft()
        self.fft.SetFFTParams(N, False, 0.0, fs)
        self.fft.SetFFTAve(ave)
        self.buf = np.zeros(N, dtype=np.complex128)
        self.pos, self.counter, self.finished = 0, 0, True
        self.dc = np.zeros(2)
        self.total = 0

    def process(self, x, cal):
        if cal:
            self.orc.spurcal(self.dc, x)                          # :886-887
        y = (x.real - self.dc[0]) + 1j * (x.imag - self.dc[1])   # :889-894
        used, i = 0, 0
        while i < len(y):
            k = min(self.N - self.pos, len(y) - i)
            self.buf[self.pos:self.pos + k] = y[i:i + k]
            self.pos += k; i += k
            if self.pos == self.N:
                self.pos = 0
                self.counter += 1
                if self.counter >= self.skip:
                    self.counter = 0
                    if self.finished:
                        self.total = self.fft.PutInDisplayFFT(self.buf)
                        self.finished = not self.gated
                        used += 1
        return used


def rate_for_skip(N, skip):
    return float(N * 10 * skip + 1)                             # SetMaxDisplayRate(10) -> skip value `skip`


@pytest.mark.parametrize("N,pkt_len,skip,gated", [
    (4096, 1444, 1, False), (4096, 1028, 3, True), (2048, 1028, 1, True), (2048, 1444, 5, False),
    (16384, 1444, 2, False), (16384, 1028, 1, True), (1024, 1444, 3, False), (1024, 1028, 1, False),
    (32768, 1444, 1, False), (8192, 1444, 1, False), (8192, 1028, 2, True)])
def test_packets_match_oracle_display_loop(oracle, N, pkt_len, skip, gated):
    import cutesdr_amd as ca
    from cutesdr_amd._capi import lib
    Cn, ave = 3, 3
    per = 240 if pkt_len == 1444 else 256
    fs = rate_for_skip(N, skip)
    rng = np.random.default_rng(N + pkt_len + skip)
    npk_calls = [int(v) for v in rng.integers(1, max(3 * N // per, 3), size=400)]
    need = (skip * 5 + 2) * N * (3 if gated else 1)                  # (the gate drops frames until ScreenUpdateDone)
    calls, tot = [], 0
    for k in npk_calls:
        calls.append(k); tot += k * per
        if tot >= need:
            break
    x = feed_signal(Cn, tot, fs, seed=N + skip, spike_channel=1)
    raw = make_packets(x, pkt_len)
    b = ca.FftBatch(Cn)
    b.set_params(N, False, 0.0, fs); b.set_ave(ave)
    b.set_display_rate(fs, 10, gated)
    refs = [OracleDisplay(oracle, N, ave, fs, skip, gated) for _ in range(Cn)]
    ddc = ca.DeviceBuffer(Cn * 16); ddc.upload(np.zeros(2 * Cn))
    dp = ca.DeviceBuffer(raw.nbytes)
    p0, frames = 0, 0
    for ci, k in enumerate(calls):
        part = np.ascontiguousarray(raw[:, p0:p0 + k])
        dp.upload(part)
        cal = ci < 3                                            # NCO spur calibration active for the first calls
        if cal:
            assert lib().csdr_ingest_spurcal_packets(0, C.c_void_p(dp.ptr), Cn, k, pkt_len, C.c_void_p(ddc.ptr), None) == 0
        got = b.put_display_packets_ptr(dp.ptr, k, pkt_len, ddc.ptr)
        want = [r.process(oracle.unpack_packets(part[c], pkt_len), cal) for c, r in enumerate(refs)]
        assert got == want[0] == want[1] == want[2], ci
        frames += got
        if gated and rng.random() < 0.5:
            b.screen_update_done()
            for r in refs:
                r.finished = True
        p0 += k
    ca.sync()
    assert frames >= 2
    np.testing.assert_allclose(ddc.download(np.float64, 2 * Cn).reshape(Cn, 2), np.stack([r.dc for r in refs]),
                               rtol=0, atol=1e-9 * 5000.0)
    for c in range(Cn):
        assert b.total_count(c) == refs[c].total
        assert_spectrum_close(b.ave_buf(c).astype(np.float64), refs[c].fft.ave_buf())
    ov, pix = b.screen_all(255, 700, 0.0, -160.0, -int(fs / 2), int(fs / 2))
    for c in range(Cn):
        want_ov, want = refs[c].fft.GetScreenIntegerFFTData(255, 700, 0.0, -160.0, -int(fs / 2), int(fs / 2))
        assert ov[c] == want_ov
        touched = pix[c] >= 0
        assert np.abs(pix[c][touched] - want[touched]).max() <= 1


@pytest.mark.parametrize("N,pkt_len", [(4096, 1444), (2048, 1028), (1024, 1444), (8192, 1028), (16384, 1444)])
def test_packets_equal_unpack_then_stream(N, pkt_len):
    """put_display_packets(dc) gives the words of csdr_ingest_unpack(dc) + put_display_stream(dc=NULL)"""
    import cutesdr_amd as ca
    Cn, per = 4, (240 if pkt_len == 1444 else 256)
    fs = rate_for_skip(N, 2)
    rng = np.random.default_rng(7)
    calls = [int(v) for v in rng.integers(1, 3 * N // per + 2, size=12)]
    x = feed_signal(Cn, sum(calls) * per, fs, seed=3)
    raw = make_packets(x, pkt_len)
    dc = np.array([[151.25, -88.5], [180.0, -107.75], [-3.0, 2.5], [0.125, 0.0]])
    a, b = ca.FftBatch(Cn), ca.FftBatch(Cn)
    for o in (a, b):
        o.set_params(N, False, 0.0, fs); o.set_ave(4); o.set_display_rate(fs, 10)
    p0 = 0
    for k in calls:
        part = raw[:, p0:p0 + k]
        y = ca.unpack_packets_batch(part, pkt_len, dc)
        assert a.put_display_packets(part, pkt_len, dc) == b.put_display_stream(y)
        p0 += k
    for c in range(Cn):
        assert a.total_count(c) == b.total_count(c) > 0
        assert np.array_equal(a.ave_buf(c).view(np.uint32), b.ave_buf(c).view(np.uint32))


@pytest.mark.parametrize("N", [2048, 4096, 8192, 512])
def test_whole_frames_equal_put_display(N):
    """put_display_stream with n a multiple of N, skip 0 and no DC gives the words of put_display"""
    import cutesdr_amd as ca
    Cn = 3
    x = feed_signal(Cn, 6 * N, 2e6, seed=11).astype(np.complex64)
    a, b = ca.FftBatch(Cn), ca.FftBatch(Cn)
    for o in (a, b):
        o.set_params(N, False, 0.0, 2e6); o.set_ave(3)
    for k in (2, 1, 3):
        part = x[:, :k * N]; x = x[:, k * N:]
        assert a.put_display_stream(part) == k
        b.put_display(part)
        for c in range(Cn):
            assert a.total_count(c) == b.total_count(c)
            assert np.array_equal(a.ave_buf(c).view(np.uint32), b.ave_buf(c).view(np.uint32))


@pytest.mark.parametrize("N,skip,ave,dc", [(4096, 7, 4, True), (2048, 1, 1, True), (16384, 3, 2, False),
                                           (1024, 1, 1, False)])
def test_call_cutting_does_not_matter(N, skip, ave, dc):
    """one call of k N + r samples gives the words of the same samples cut into many ragged calls"""
    import cutesdr_amd as ca
    Cn = 3
    fs = rate_for_skip(N, skip)
    n = 40 * N + 777
    x = feed_signal(Cn, n, fs, seed=5).astype(np.complex64)
    d = np.array([[12.5, -3.25]] * Cn) if dc else None
    a, b = ca.FftBatch(Cn), ca.FftBatch(Cn)
    for o in (a, b):
        o.set_params(N, False, 0.0, fs); o.set_ave(ave); o.set_display_rate(fs, 10)
    ka = a.put_display_stream(x, d)
    rng = np.random.default_rng(N)
    kb, p = 0, 0
    while p < n:
        k = int(min(n - p, rng.integers(1, 3 * N)))
        kb += b.put_display_stream(x[:, p:p + k], d)
        p += k
    assert ka == kb == (40 if skip <= 1 else 40 // skip)
    for c in range(Cn):
        assert a.total_count(c) == b.total_count(c) == ka
        assert np.array_equal(a.ave_buf(c).view(np.uint32), b.ave_buf(c).view(np.uint32))
    # the carried partial frame is the same too: one more frame completes identically
    tail = feed_signal(Cn, N, fs, seed=6).astype(np.complex64)
    a.set_display_rate(1.0, 10); b.set_display_rate(1.0, 10)             # skip 0 from here: the next frame is used
    assert a.put_display_stream(tail, d) == b.put_display_stream(tail, d) == 1
    for c in range(Cn):
        assert np.array_equal(a.ave_buf(c).view(np.uint32), b.ave_buf(c).view(np.uint32))


def test_no_frame_leaves_spectrum_untouched():
    import cutesdr_amd as ca
    N, Cn = 4096, 2
    b = ca.FftBatch(Cn)
    b.set_params(N, False, 0.0, 2e6); b.set_ave(2)
    x = feed_signal(Cn, 3 * N, 2e6, seed=9).astype(np.complex64)
    x[0, 10] = 32700.0                                                       # channel 0 overloads in the first frame
    assert b.put_display_stream(x[:, :N + 100]) == 1
    ov0, _ = b.screen_all(255, 100, 0.0, -160.0, -1000, 1000)
    assert list(ov0) == [True, False]
    before = [b.ave_buf(c).copy() for c in range(Cn)]
    assert b.put_display_stream(x[:, N + 100:2 * N - 5]) == 0                # completes no frame
    for c in range(Cn):
        assert np.array_equal(b.ave_buf(c), before[c]) and b.total_count(c) == 1
    ov1, _ = b.screen_all(255, 100, 0.0, -160.0, -1000, 1000)
    assert np.array_equal(ov0, ov1)
    b.stream_reset()                                                         # StartSdr: the partial frame is dropped
    assert b.put_display_stream(x[:, :N - 1]) == 0
    assert b.put_display_stream(x[:, N - 1:N]) == 1
    b2 = ca.FftBatch(Cn)
    b2.set_params(N, False, 0.0, 2e6); b2.set_ave(2)
    b2.put_display(x[:, :N])
    b2.put_display(x[:, :N])
    for c in range(Cn):
        assert np.array_equal(b.ave_buf(c).view(np.uint32), b2.ave_buf(c).view(np.uint32))


@pytest.mark.parametrize("pkt_len", [1028, 1444])
def test_spurcal_packets_bit_equal(pkt_len):
    import cutesdr_amd as ca
    from cutesdr_amd._capi import lib
    Cn, per, npk = 5, (240 if pkt_len == 1444 else 256), 333
    x = feed_signal(Cn, npk * per, 2e6, seed=21)
    raw = make_packets(x, pkt_len)
    dc0 = np.array([[0.0, 0.0], [10.0, -5.0], [151.0, -90.0], [-1.5, 3.0], [7.0, 7.0]])
    got = ca.spurcal_packets_batch(raw, pkt_len, dc0)
    y = ca.unpack_packets_batch(raw, pkt_len)
    dy = ca.DeviceBuffer(y.nbytes); dy.upload(y)
    dd = ca.DeviceBuffer(Cn * 16); dd.upload(dc0)
    assert lib().csdr_ingest_spurcal(0, C.c_void_p(dy.ptr), y.shape[1], Cn, y.shape[1], C.c_void_p(dd.ptr), None) == 0
    ca.sync()
    want = dd.download(np.float64, 2 * Cn).reshape(Cn, 2)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert not np.array_equal(got, dc0)


def test_set_params_rederives_skip_from_its_rate():
    """SetFftSize calls SetMaxDisplayRate at m_SampleRate, the rate SetFFTParams gets: the skip value follows set_params"""
    import cutesdr_amd as ca
    N, Cn = 2048, 2
    b = ca.FftBatch(Cn)
    b.set_params(N, False, 0.0, rate_for_skip(N, 5)); b.set_display_rate(rate_for_skip(N, 5), 10)
    x = feed_signal(Cn, 20 * N, 1e6, seed=4).astype(np.complex64)
    assert b.put_display_stream(x) == 4                                      # skip 5
    b.set_params(N, False, 0.0, rate_for_skip(N, 2))                         # same size, new rate: skip 2, counter 0
    assert b.put_display_stream(x) == 10
    b.set_params(4096, False, 0.0, rate_for_skip(N, 2))                      # twice the size at that rate: skip 1
    assert b.put_display_stream(x) == 10
