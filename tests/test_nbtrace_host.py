"""nbtrace_ref.py, the restatement of the blanker with its test-bench trace, pinned to the reference's compiled code
(no GPU).  oracle.ref.CNoiseProc.ProcessBlanker is fed ONE sample per call: every call ends in DisplayData(1,
m_TestBenchDataBuf, rate, PROFILE_7) (noiseproc.cpp:175; with the blanker off: of pOutData, :127), which the recording
test bench keeps as (profile, n, complex, rate, first value) -- m_TestBenchDataBuf[0].re of that sample.  The call's
output is the delayed sample or (0, 0), which pins the imaginary part's operands and the blanking decision."""
import numpy as np
import pytest

import nbtrace_ref as N

# (on, sample rate, threshold, width us, samples, impulses): the second has two impulses closer together than the width
SETTINGS = [(True, 100e3, 20.0, 50.0, 3000, [(700, 30000, -5), (1500, -32767, 32767), (2400, 12, 28000)]),
            (True, 500e3, 10.0, 100.0, 6000, [(2600, 32767, 0), (2620, 0, -32767), (4000, -20000, 20000)]),
            (False, 100e3, 20.0, 50.0, 500, [(100, 30000, 0)])]


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as r
    if not r.tree_present() and r.build() is None:
        pytest.skip("neither oracle/_ref/libcutesdr_ref.so nor the reference tree is here")
    assert r.available()
    return r


@pytest.mark.parametrize("k", range(len(SETTINGS)))
def test_restatement_is_the_compiled_reference(ref, k):
    on, fs, thresh, width, n, impulses = SETTINGS[k]
    x = N.datagram_like(n, 11 + k, impulses=impulses)
    mine = N.RefNoiseProc()
    mine.SetupBlanker(on, thresh, width, fs)
    out, tb, blanked = mine.ProcessBlanker(x)
    theirs = ref.CNoiseProc()
    theirs.SetupBlanker(on, thresh, width, fs)
    ref.clear_tap_calls()
    got_out = np.concatenate([theirs.ProcessBlanker(x[i:i + 1]) for i in range(n)])
    calls = [c for c in ref.tap_calls() if c[0] == 7]
    ref.clear_tap_calls()
    assert len(calls) == n and all(c[1] == 1 and c[2] and c[3] == fs for c in calls)
    got_re = np.array([c[4] for c in calls], dtype=np.float64)
    assert got_re.view(np.uint64).tolist() == tb.real.copy().view(np.uint64).tolist()       # bit for bit
    assert got_out.view(np.uint64).tolist() == out.view(np.uint64).tolist()
    if on:
        # both branches of re: blanked samples (exactly 0) and the moving sum over the ratio (never 0 on this input)
        assert 0 < blanked.sum() < n and (tb.real[blanked] == 0.0).all() and (tb.real[~blanked] > 0.0).all()
        d = mine.m_DelaySamples + 1
        assert (tb.imag[d:] == x.real[:-d] + x.imag[:-d]).all() and (tb.imag[:d] == 0.0).all()
    else:
        assert not blanked.any() and (tb == x).all()


def test_close_impulses_extend_the_blank_window():
    """the second setting's impulses are 20 samples apart, the width 49 samples ((int)(100 * 1e-6 * 500e3) in fp64):
    one stretch of 20 + 49 blanked samples"""
    on, fs, thresh, width, n, impulses = SETTINGS[1]
    r = N.RefNoiseProc()
    r.SetupBlanker(on, thresh, width, fs)
    blanked = r.ProcessBlanker(N.datagram_like(n, 12, impulses=impulses))[2]
    assert r.m_WidthSamples == 49 and blanked[2600:2669].all() and not blanked[2669] and not blanked[2599]


def test_threshold_zero_divides_by_zero_as_ieee_does():
    r = N.RefNoiseProc()
    r.SetupBlanker(True, 0.0, 50.0, 100e3)
    tb = r.ProcessBlanker(np.array([0.0, 3 + 4j, 1.0]))[1]
    assert np.isnan(tb.real[0]) and np.isposinf(tb.real[1]) and np.isposinf(tb.real[2])


def test_the_gpu_tests_shapes_reach_the_forms_they_name():
    """on the host's own rules (csdr__host_nb_*, no GPU): the four receivers of test_nbtrace_gpu.py's object A take the
    sample form with the ring, the 100 kS/s receiver of object B the two-stream form, and the 3 * 65536 + 1000 call is
    cut into three segments in both"""
    import ctypes as C
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__host_nb_segments.restype = None
    L.csdr__host_nb_segments.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.csdr__host_nb_form.restype = C.c_int
    L.csdr__host_nb_form.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    NB_SAMPLES, NB_SAMPLES_RING = 0, 1
    for rates, on, form in (([500e3, 2e6, 2e6, 500e3], [1, 1, 1, 0], NB_SAMPLES_RING), ([100e3], [1], NB_SAMPLES)):
        ch = len(rates)
        a_on = (C.c_int * ch)(*on)
        a_mag = (C.c_int * ch)(*[int(N.MAGAVE_TIME * fs) for fs in rates])
        a_int = (C.c_int * ch)(*([0] * ch))
        for pkt_len in (0, 1028, 1444):
            assert L.csdr__host_nb_form(0, pkt_len, ch, a_on, a_mag, a_int, 1, 1) == form
        nseg, seg_len = C.c_int(), C.c_int()
        L.csdr__host_nb_segments(3 * 65536 + 1000, ch, 0, int(form == NB_SAMPLES_RING), C.byref(nseg), C.byref(seg_len))
        assert nseg.value == 3 and seg_len.value % 2048 == 0
