"""The int16 overloads of the batch test-bench scope (csdr_scope_batch_put_mono16 / _put_stereo16) on the device against
scope16_ref.py, the restatement of gui/testbench.cpp:702-814.

Time view: scope_ref's scenario -- 16 receivers, its five widths, its uneven cuts drawn from {1, 7, 256, 513, 1000}, its
mid-stream events -- on the rows cast to int16; emits, screens and final states exact.  The cuts are odd and 1-sample
ones too, so the mono overload's trigger read pBuf[i<<1] falls past the call's n samples (deviation (7): 0 there).
FFT view: test_scope_fft_gpu.py's receivers, cuts, driver and tolerances on int16 rows -- (x, x) frames mapped as real
for mono, (re, im) mapped as complex for stereo."""
import numpy as np
import pytest

import scope16_ref as S
import scope_fft_ref as F
import scope_ref as R
import test_scope_fft_gpu as TF
from test_scope_gpu import GpuBatch

pytestmark = pytest.mark.gpu


class Gpu16(GpuBatch):
    """cutesdr_amd.ScopeBatch fed with int16 rows: numpy [channels, T] (mono) or [channels, T, 2] (stereo)"""

    def put(self, rows, pos, n, rates):
        import torch
        if self.src is not rows:
            self.src, self.t = rows, torch.from_numpy(rows).cuda()
            self.before = self.t.clone()
        stereo = rows.ndim == 3
        self.s.put16_ptr(self.t.data_ptr() + pos * (4 if stereo else 2), self.t.stride(0) // (2 if stereo else 1), n, rates,
                         torch.cuda.current_stream().cuda_stream, stereo=stereo)


# ------------------------------------------------------------------------------------------------- the time view
@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("stereo", [False, True], ids=["mono16", "stereo16"])
def test_parity(stereo, k):
    import torch
    d = Gpu16()
    totals, past = S.check(d, k, stereo)
    print("screens of the 16 receivers, width %d:" % R.CONFIGS[k][0], totals, "trigger reads past n:", past)
    c = R.cuts()
    assert 1 in c and any(n % 2 for n in c)
    assert totals[R.UNREACHED] == 0 and totals[R.IDLE] == 0 and sum(1 for t in totals if t) >= 8, totals
    if stereo:
        R.check_counts(k, totals)
        assert any(any(d.screen(c)[1]) for c in range(16)) and past == 0
    else:
        assert past > 100, past                          # 2i >= n happened, in the restatement the device just matched
    torch.cuda.synchronize()
    assert torch.equal(d.t, d.before)                    # the rows are never written


@pytest.mark.parametrize("stereo", [False, True], ids=["mono16", "stereo16"])
def test_slots_in_mid_stream(stereo):
    S.check(Gpu16(), 0, stereo, "mid", R.mid_stream_events(0))


def test_mono_trigger_reads_2i():
    """the same samples through put_real (as fp32) and through put_mono16: the ring contents are the same samples, but
    the trigger looks at pBuf[2i], so a triggered receiver's screen is another stretch of the stream"""
    k = 0
    rows = S.rows16(False)
    mono, real = Gpu16(), GpuBatch()
    frows = rows.astype(np.float32)
    for d, x in ((mono, rows), (real, frows)):
        R.configure(d, k)
        R.run(d, x, k, R.cuts())
    rx = 4                                               # PSINGLE: its one screen hangs on the FIRST crossing after the reset,
    assert mono.totals()[rx] == 1 and real.totals()[rx] == 1    # which pBuf[2i] and pBuf[i] reach at different emissions
    assert mono.screen(rx) != real.screen(rx)
    assert mono.screen(rx) == S.trace(k, False)[4][rx]
    assert not any(mono.screen(rx)[1])                   # the mono overload writes 0 into the second ring


def test_rejects_bad_arguments():
    import torch
    import cutesdr_amd as ca
    rows = torch.zeros((2, 64), dtype=torch.int16, device="cuda")
    s = ca.ScopeBatch(2)
    with pytest.raises(ca._capi.CsdrError):
        s.put16_ptr(rows.data_ptr(), 64, [65, 0], 48000.0)                      # n > stride
    with pytest.raises(ca._capi.CsdrError):
        s.put16_ptr(rows.data_ptr() + 2, 31, [8, 8], 48000.0, stereo=True)      # pairs need 4-byte alignment
    with pytest.raises(ca._capi.CsdrError):
        s.put16_ptr(rows.data_ptr() + 1, 32, [8, 8], 48000.0)                   # int16 needs 2
    s.put16_ptr(rows.data_ptr() + 2, 63, [8, 8], 48000.0)                       # an odd offset and stride are fine for mono
    s.put_mono16(rows, [64, 0], [48000.0, 0.0])                                 # a rate of 0 is not looked at where n = 0
    assert s.get_emits().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------- the FFT view
class GpuFft16(TF.Gpu):
    put = Gpu16.put


def rows_fft(stereo):
    x = TF.rows_for(True)                                # tones at -20 and -30.5 dBFS plus noise at -40 dBFS
    if not stereo:
        return np.trunc(x.real).astype(np.int16)
    return np.stack([np.trunc(x.real), np.trunc(x.imag)], axis=-1).astype(np.int16)


@pytest.mark.parametrize("w,h", [(100, 100), (700, 255)])
@pytest.mark.parametrize("stereo", [False, True], ids=["mono16", "stereo16"])
def test_fft_view(oracle, stereo, w, h):
    """bels within assert_spectrum_close's classes of the oracle's on (x, x) / (re, im) frames, every pixel inside the
    interval those tolerances map to, the peak hold over every used frame (at least five per receiver); the mono
    screen starts at 0 Hz (mapped as real), the stereo one at -span/2"""
    d, ref = GpuFft16(), S.RefFftBatch16(oracle, TF.CH)
    TF.configure(d, w, h); TF.configure(ref, w, h)
    drawn = TF.drive(d, ref, rows_fft(stereo), TF.cuts(), [r[0] for r in TF.RX])
    assert drawn >= 60 and all(r.total >= 5 for c, r in enumerate(ref.r) if c != TF.IDLE), drawn
    for c, r in enumerate(ref.r):
        if c != TF.IDLE:
            assert d.s.get_fft_screen(c)[2] == stereo and r.fft_cpx == stereo, c
    if not stereo:                                       # (x, x): the frame the oracle saw really had both parts
        assert all((r.m_FftInBuf.real == r.m_FftInBuf.imag).all() and r.m_FftInBuf.real.any() for c, r in enumerate(ref.r) if c != TF.IDLE)
