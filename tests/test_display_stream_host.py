"""CPU tests of the display stream's host logic (no GPU): the frame planner behind csdr_fft_batch_put_display_stream /
_packets against a literal transcription of CSdrInterface::ProcessIQData's display loop (reference
interface/sdrinterface.cpp:889-907), the skip value of SetMaxDisplayRate (sdrinterface.h:112-114), and the no-GPU
failure of the new entry points."""
import ctypes as C
import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_display_plan.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]
    lib.csdr__host_display_plan.restype = None
    lib.csdr__host_display_skip_value.argtypes = [C.c_double, C.c_int, C.c_int]
    return lib


class RefDisplayLoop:
    """sdrinterface.cpp:889-907, sample by sample; a frame is identified by the stream index of its first sample."""

    def __init__(self, N, skip, gated):
        self.N, self.skip = N, skip
        self.fft_buf_pos = 0                 # m_FftBufPos counts doubles: 2 per complex sample
        self.counter = 0                     # m_DisplaySkipCounter
        self.finished = True                 # m_ScreenUpateFinished
        self.gated = gated
        self.consumed = 0

    def process(self, n):
        used = []
        for i in range(2 * n):               # for(int i=0; i<Length; i++)
            self.fft_buf_pos += 1
            if self.fft_buf_pos >= self.N * 2:
                self.fft_buf_pos = 0
                self.counter += 1
                if self.counter >= self.skip:
                    self.counter = 0
                    if self.finished:
                        used.append(self.consumed + i // 2 + 1 - self.N)    # PutInDisplayFFT(m_DataBuf)
                        if self.gated:
                            self.finished = False                          # (ungated: the GUI answers at once)
        self.consumed += n
        return used


def plan(L, state, n, N):
    s = (C.c_int * 5)(*state)
    out = (C.c_longlong * 8)()
    L.csdr__host_display_plan(s, n, N, out)
    return list(out)


@pytest.mark.parametrize("N", [8, 32, 128])
@pytest.mark.parametrize("skip", [0, 1, 2, 7, 48])
@pytest.mark.parametrize("gated", [False, True])
def test_planner_matches_reference_loop(L, N, skip, gated):
    rng = np.random.default_rng(1000 * N + 10 * skip + gated)
    ref = RefDisplayLoop(N, skip, gated)
    state = [0, skip, 0, int(gated), 1]
    pos_abs = 0
    for call in range(300):
        if gated and rng.random() < 0.3:
            ref.finished = True                               # ScreenUpdateDone()
            state[4] = 1
        rem = N - state[0]
        n = int(rng.choice([rng.integers(1, max(rem, 2)), rng.integers(1, 3 * N + 1), rem, 0]))
        want = ref.process(n)
        start, step, count, P, sk, cnt, gt, rd = plan(L, state, n, N)
        got = [pos_abs + start + k * step for k in range(count)]
        assert got == want, (call, n, state)
        assert step % N == 0 and start >= -state[0]
        pos_abs += n
        state = [P, sk, cnt, gt, rd]
        assert P * 2 == ref.fft_buf_pos
        assert cnt == ref.counter
        assert bool(rd) == ref.finished
        if count:                                              # every used frame lies inside carry + this call
            assert start + (count - 1) * step + N <= n


def test_planner_long_call(L):
    """one call of k N + r samples uses the same frames as the same samples cut into many calls"""
    N, skip = 64, 7
    start, step, count, P, _, cnt, _, _ = plan(L, [5, skip, 3, 0, 1], 100 * N + 17, N)
    ref = RefDisplayLoop(N, skip, False)
    ref.fft_buf_pos, ref.counter = 10, 3                       # 5 samples carried, counter at 3
    want = ref.process(100 * N + 17)
    assert [start + k * step for k in range(count)] == want
    assert P == (5 + 100 * N + 17) % N and cnt == ref.counter


def test_skip_value_truncates_like_reference(L):
    f = L.csdr__host_display_skip_value
    assert f(2e6, 4096, 10) == 48                              # 48.83
    assert f(1e5, 65536, 10) == 0                              # 0.15: every frame
    assert f(2e6, 2048, 10) == 97
    assert f(1.2e6, 16384, 10) == 7
    assert f(62500.0, 4096, 15) == 1
    for fs, n, r in [(2e6, 4096, 10), (1.5e6, 8192, 25), (250e3, 512, 3)]:
        assert f(fs, n, r) == int(fs / (n * r))


def test_new_entry_points_fail_cleanly_without_gpu(L):
    from cutesdr_amd import _capi
    if L.csdr_device_count() > 0:
        pytest.skip("GPU present")
    EINVAL, EHIP = _capi.CSDR_EINVAL, _capi.CSDR_EHIP
    assert not L.csdr_fft_batch_create(0, 4)
    assert L.csdr_fft_batch_set_display_rate(None, 2e6, 10, 0) == EINVAL
    assert L.csdr_fft_batch_screen_update_done(None) == EINVAL
    assert L.csdr_fft_batch_stream_reset(None) == EINVAL
    buf = (C.c_ubyte * 4096)()
    assert L.csdr_fft_batch_put_display_stream(None, C.addressof(buf), 8, 8, None, None) == EINVAL
    assert L.csdr_fft_batch_put_display_packets(None, C.addressof(buf), 2, 1444, None, None) == EINVAL
    dc = (C.c_double * 2)()
    assert L.csdr_ingest_spurcal_packets(0, C.addressof(buf), 1, 2, 1444, C.addressof(dc), None) == EHIP
    assert L.csdr_ingest_spurcal_packets(0, C.addressof(buf), 1, 2, 1000, C.addressof(dc), None) == EINVAL
    assert L.csdr_ingest_spurcal_packets(0, C.addressof(buf) + 2, 1, 2, 1028, C.addressof(dc), None) == EINVAL
    import cutesdr_amd
    with pytest.raises(_capi.CsdrError):
        cutesdr_amd.FftBatch(2)
