"""The fp64 oracle (oracle/cutesdr_oracle.c, this project's restatement) against the reference's own dsp/ code compiled
unmodified (oracle/ref.py -> oracle/_ref/libcutesdr_ref.so), on the CPU, same inputs and same calls on both.

Rules (the bounds are derived, HISTORY.md "Oracle against the reference's compiled code" holds the measured maxima):
  * everything without an FFT in it: BIT EQUALITY of the fp64 words (np.array_equal), counts equal.  Both sides are
    compiled without contraction or fast-math and sum in the same order, so nothing else is acceptable;
  * FFT stages (the oracle's radix-2 against the reference's Ooura radix-4): FFT_EPS = 1e-13 * max|x| per sample for the
    scaled round trip of the filter, * N for the unscaled transforms -- about 2 log2 N rounding steps of 1.1e-16 with a
    decade of room;
  * the whole CDemodulator: counts, S-meter, squelch decisions and the recorded PROFILE_* calls equal; audio burst by
    burst CHAIN_EPS = 1e-9 of full scale (1/20000 of the 2e-5 the GPU is held to; about 1e7 fp64 roundings on a chain of
    1e4 operations per sample with feedback) -- AM / SSB / CW from burst 0, SAM from burst 2, FM from burst 14; SAM
    bursts 0 and 1 and FM bursts 1..5 behind the pull-in inside tests/startup_bounds.py's numbers, unchanged (the first
    check of those numbers against the real reference).

Skipped only where neither the library nor the reference tree exists; where the tree exists a missing library fails.
Every comparison prints its figure (pytest -s)."""
import numpy as np
import pytest

import startup_bounds as SB
from util_signals import tones_plus_noise, fm_carrier, am_carrier, FULL_SCALE
from test_postchain_gpu import info, make_input, level_steps, burst_errors
from test_chain_parity_gpu import MODES, chain_input
from test_frontend_gpu import impulsive
from cutesdr_amd import _build

FFT_EPS = 1e-13
CHAIN_EPS = 1e-9 * FULL_SCALE
RADIO_RATE = 80e6 / 130.0
# The S-meter behind the FFT filter cannot be EQUAL: it averages 10 log10 |z|^2 sample by sample (smeter.cpp:76-79), so a
# filter-output difference e moves one sample's term by 8.7 e / |z| dB and the reading by at most alpha = 1.6e-3 (the 10 ms
# attack at 62.5 kS/s) of that.  With e <= FFT_EPS * max|x| a single sample moves the reading by 1e-6 dB only if it lies
# 180 dB below the input's peak; the test signals' in-band noise floor is 85 dB below it.  Measured: 1.1e-8 dB (LSB), 4e-14 elsewhere.
SMETER_EPS = 1e-6


@pytest.fixture(scope="module")
def R():
    from oracle import ref
    if not ref.tree_present() and ref.build() is None:
        pytest.skip("neither oracle/_ref/libcutesdr_ref.so nor the reference tree is here")
    assert ref.available(), "the reference tree is here, so the library must build"
    return ref


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), (what, "first differing word", int(np.flatnonzero(a != b)[0]), float(np.abs(a - b).max()))


def fig(what, value):
    print("OVR %s: %.3g" % (what, value))


# ------------------------------------------------------------------------------------------------ construction
def test_zeroed_construction_gives_the_same_initial_state(O, R):
    """The reference's constructors leave members unset (ref_shim.cpp lists them); constructed into zeroed storage they
    read as zero, and that is the oracle's initial state: before any setter, the getters and a first call agree, and a
    CDemodulator's first SetDemod (which deletes m_pFmDemod, never initialised) is safe, 40 objects in a row."""
    for _ in range(40):
        d = R.CDemodulator(2048)
        d.SetDemod(2, info(R))
    a, b = O.CDemodulator(2048), R.CDemodulator(2048)
    assert a.buf_limit() == b.buf_limit() == 1000 and a.GetOutputRate() == b.GetOutputRate() == 48000.0
    assert a.GetSMeterAve() == b.GetSMeterAve() and a.GetSMeterPeak() == b.GetSMeterPeak()
    for o, mod in ((a, O), (b, R)):                        # m_InputRate reads as 0: SetDataRate(0, bw) builds no stage
        o.SetDemod(3, info(mod, **MODES["USB"][1]))
    assert a.GetOutputRate() == b.GetOutputRate() and a.buf_limit() == b.buf_limit()
    a, b = O.CDownConvert(), R.CDownConvert()
    assert a.nco_freq() == b.nco_freq() == 0.0 and a.stages() == b.stages() == []
    x = tones_plus_noise(1, 512, 1e5, [1e3])
    # The one place where the two initial states differ, by the oracle's own choice (HISTORY.md): the reference's
    # constructor leaves m_OscCos / m_OscSin unset until the first SetFrequency (downconvert.cpp:60-73, 104-105); read
    # as zero they stop the oscillator at once.  The oracle starts them as SetFrequency(0) would.  No chain gets there:
    # CDemodulator's constructor calls SetDemodFreq (demodulator.cpp:59).
    assert not b.ProcessData(x).any()
    c = R.CDownConvert(); c.SetFrequency(0.0)
    same(a.ProcessData(x), c.ProcessData(x), "the oracle's fresh down-converter is the reference's after SetFrequency(0)")
    a, b = O.CFmDemod(62500.0), R.CFmDemod(62500.0)        # m_SquelchThreshold unset: 0 forces the squelch shut
    x = fm_carrier(1024, 62500.0, 300.0, dbfs=-6.0)
    same(a.ProcessData(x, 5000.0), b.ProcessData(x, 5000.0), "FM before SetSquelch")
    assert a.squelched() and b.squelched()
    a, b = O.CSMeter(), R.CSMeter()
    assert a.GetAve() == b.GetAve() and a.GetPeak() == b.GetPeak()
    a, b = O.CAgc(), R.CAgc()
    for o in (a, b):
        o.SetParameters(False, False, 0, 0, 0, 0, 0.0)     # all zero: equal to the zeroed members, the reference returns early
    same(a.ProcessData(x), b.ProcessData(x), "AGC whose first SetParameters is all zeros")


def test_the_callers_array_is_never_written(R):
    """CDownConvert::ProcessData, CFastFIR::ProcessData and CFft::PutInDisplayFFT work in place; the binding hands them
    a private copy"""
    x = tones_plus_noise(2, 4096, 2e6, [1e5]); keep = x.copy()
    dc = R.CDownConvert(); dc.SetDataRate(2e6, 15000.0); dc.SetFrequency(-1e5); dc.ProcessData(x)
    ff = R.CFastFIR(2048); ff.SetupParameters(-5000, 5000, 0, 62500.0); ff.ProcessData(x)
    f = R.CFft(); f.SetFFTParams(4096, False, 0.0, 2e6); f.PutInDisplayFFT(x); f.FwdFFT(x)
    d = R.CDemodulator(2048); d.SetInputSampleRate(2e6); d.SetDemod(0, info(R, **MODES["AM"][1])); d.ProcessData(x); d.process_append(x)
    a = R.CAgc(); a.SetParameters(True, False, -100, 30, 0, 200, 62500.0); a.ProcessData(x); a.ProcessData(x.real.copy())
    nb = R.CNoiseProc(); nb.SetupBlanker(True, 50.0, 2.0, 2e6); nb.ProcessBlanker(x)
    R.CAmDemod(31250.0).ProcessData(x); R.CSamDemod(31250.0).ProcessData(x); R.CFmDemod(62500.0).ProcessData(x, 5000.0); R.ssb_demod(x)
    assert np.array_equal(x, keep)


def test_calls_beyond_the_fixed_buffers_are_refused_not_forwarded(O, R):
    dc, oc = R.CDownConvert(), O.CDownConvert()
    dc.SetDataRate(500e3, 10000.0); oc.SetDataRate(500e3, 10000.0)
    assert dc.stages() == oc.stages() == [11, 15, 23, 51]
    big = np.zeros(65536, dtype=np.complex128)
    assert len(oc.ProcessData(big)) == 0                       # the oracle refuses: 32768 samples into the 15-tap stage's scratch
    with pytest.raises(ValueError):
        dc.ProcessData(big)
    assert len(dc.ProcessData(big[:32768])) == 2048            # the longest call that fits
    with pytest.raises(ValueError):
        R.CNoiseProc().ProcessBlanker(np.zeros(4097, dtype=np.complex128))
    with pytest.raises(ValueError):
        R.CNoiseProc().SetupBlanker(True, 50.0, 2.0, 10e6)     # 5 ms > 32768 entries
    with pytest.raises(ValueError):
        R.CFmDemod(62500.0).ProcessData(np.zeros(16385, dtype=np.complex128), 5000.0)
    r = R.CFractResampler()
    with pytest.raises(ValueError):
        r.Resample(np.zeros(10), 1.0)                          # before Init there is no input buffer
    r.Init(1000)
    with pytest.raises(ValueError):
        r.Resample(np.zeros(1001), 1.0)
    f = R.CFft(); f.SetFFTParams(512, False, 0.0, 1.0)
    with pytest.raises(ValueError):
        f.PutInDisplayFFT(np.zeros(513, dtype=np.complex128))
    with pytest.raises(ValueError):
        f.GetScreenIntegerFFTData(100, 513, 0.0, -100.0, -1, 1)
    for make in (R.CFastFIR, R.CDemodulator):                  # CONV_FFT_SIZE is 2048 and nothing else
        with pytest.raises(ValueError):
            make(4096)
    d = R.CDemodulator(2048); d.SetInputSampleRate(60e6); d.SetDemod(2, info(R))
    assert d.buf_limit() > R.limit("MAX_INBUFSIZE")
    with pytest.raises(ValueError):
        d.ProcessData(np.zeros(256, dtype=np.complex128))


# ------------------------------------------------------------------------------------------------ bit equality
NINE = (3, 3, 11, 11, 11, 11, 15, 23, 47)
DC_CASES = [(2e6, 15000.0), (2e6, 1000.0), (10e6, 15000.0), (1.8e6, 20000.0), (500e3, 10000.0), _build.all_dc_plans()[NINE]]


@pytest.mark.parametrize("rate,bw", DC_CASES, ids=lambda v: "%g" % v)
def test_downconvert_words(O, R, rate, bw):
    """3 calls of 32768 samples (16384 where the first stage is a buffered half band), the CW offset set, a retune
    between calls"""
    a, b = O.CDownConvert(), R.CDownConvert()
    for o in (a, b):
        o.SetCwOffset(700.0)
        assert o.SetDataRate(rate, bw) == rate / (1 << len(o.stages()))
        o.SetFrequency(-0.05 * rate)
    assert a.stages() == b.stages() and a.nco_freq() == b.nco_freq() == -0.05 * rate + 700.0
    n = 16384 if rate == 500e3 else 32768
    x = tones_plus_noise(3, 3 * n, rate, [0.05 * rate + 500.0, -0.2 * rate])
    for i in range(3):
        if i == 2:
            a.SetFrequency(0.11 * rate); b.SetFrequency(0.11 * rate)
        ya, yb = a.ProcessData(x[i * n:(i + 1) * n]), b.ProcessData(x[i * n:(i + 1) * n])
        assert len(ya) == n >> len(a.stages())
        same(ya, yb, ("down-converter", rate, bw, i))


def test_set_data_rate_over_every_plan(O, R):
    """rate returned, stage list and NCO frequency (the CW offset is added once more by every SetDataRate) for every
    rate / bandwidth pair of the plan table, on ONE object each, so every call also rebuilds from the previous plan"""
    plans = _build.all_dc_plans()
    assert len(plans) == 164
    a, b = O.CDownConvert(), R.CDownConvert()
    a.SetCwOffset(-700.0); b.SetCwOffset(-700.0)
    pairs = list(plans.items()) + [(None, (r, w)) for r in _build.RADIO_RATES + _build.MORE_RATES for w in _build.DEMOD_BWS]
    tenth = 0
    for plan, (rate, bw) in pairs:
        ra = a.SetDataRate(rate, bw)
        try:
            rb = b.SetDataRate(rate, bw)
        except ValueError:                   # eleven stages or more: the reference would write behind its list
            assert len(a.stages()) == 9
            tenth += 1
            b.SetCwOffset(0.0); b.SetFrequency(a.nco_freq()); b.SetCwOffset(-700.0)      # (keep the two NCO frequencies in step)
            continue
        sa, sb = a.stages(), b.stages()
        assert a.nco_freq() == b.nco_freq()
        if len(sb) == 10:
            # A DIFFERENCE, kept (HISTORY.md): the reference's loop (downconvert.cpp:127-166) has no bound on the stage
            # count; ten stages fill m_pDecimatorPtrs[MAX_DECSTAGES] to its end, the list loses its terminating null and
            # ProcessData (:252) walks past the array.  The oracle and the product stop at nine stages, which is the
            # reference's plan without its last stage, at twice its rate; the binding refuses to process with ten.
            tenth += 1
            assert sa == sb[:9] and ra == 2.0 * rb, (plan, rate, bw)
            with pytest.raises(ValueError):
                b.ProcessData(np.zeros(1024, dtype=np.complex128))
            continue
        assert ra == rb and sa == sb, (plan, rate, bw, sa, sb)
        if plan is not None:
            assert tuple(sb) == plan and rb == rate / (1 << len(plan)), (plan, rate, bw)
    fig("rate / bandwidth pairs at which the reference builds a tenth stage, of %d" % len(pairs), tenth)
    assert 0 < tenth < len(pairs) // 4


@pytest.mark.parametrize("rate", [1.0, 1.6276041666666667, 0.7312, 2.5])
def test_resampler_words_all_overloads(O, R, rate):
    rng = np.random.default_rng(11)
    x = 8000 * rng.standard_normal(3 * 2048)
    xc = x + 8000j * rng.standard_normal(3 * 2048)
    for data, gain in ((x, None), (xc, None), (x, 1.7), (xc, 0.9)):
        a, b = O.CFractResampler(), R.CFractResampler()
        a.Init(4096); b.Init(4096)
        for i in range(3):
            part = data[i * 2048:(i + 1) * 2048]
            same(a.Resample(part, rate, gain), b.Resample(part, rate, gain), ("resampler", rate, gain, i))


def test_resampler_words_rate_varies_per_call(O, R):
    """the sequence of test_resampler_rate_varies_per_call_like_the_sound_sink, both int16 and float outputs"""
    for gain in (10 ** ((80 - 99.0) / 39.2), None):
        rng = np.random.default_rng(21)
        a, b = O.CFractResampler(), R.CFractResampler()
        a.Init(8192); b.Init(8192)
        total = 0
        for k in range(40):
            n = int(rng.integers(200, 1200))
            x = 9000.0 * np.sin(2 * np.pi * 0.01 * (np.arange(n) + total)) + 200.0 * rng.standard_normal(n)
            total += n
            rate = 62500.0 / 48000.0 * (1.0 + 2.38e-7 * float(rng.integers(-2000, 2000)))
            same(a.Resample(x, rate, gain), b.Resample(x, rate, gain), ("resampler", k, gain))


@pytest.mark.parametrize("fs,thresh,width", [(2e6, 50.0, 2.0), (2e6, 20.0, 100.0), (500e3, 80.0, 3000.0), (6e6, 35.0, 10.0), (2e6, 40.0, 2040.0)])
def test_blanker_words(O, R, fs, thresh, width):
    a, b = O.CNoiseProc(), R.CNoiseProc()
    x = impulsive(int(fs) % 1000 + int(width), 120000, fs)
    same(a.ProcessBlanker(x[:3000]), b.ProcessBlanker(x[:3000]), "constructed off: data passes")
    same(a.ProcessBlanker(x[:3000]), x[:3000], "off")
    a.SetupBlanker(True, thresh, width, fs); b.SetupBlanker(True, thresh, width, fs)
    blanked, pos = 0, 0
    for n in [240, 4096, 1, 4095, 17] + [4096] * 26:           # ragged calls inside the reference's 4096-sample limit
        ya, yb = a.ProcessBlanker(x[pos:pos + n]), b.ProcessBlanker(x[pos:pos + n]); pos += n
        same(ya, yb, ("blanker", fs, thresh, width, pos))
        blanked += int((yb == 0).sum())
    assert 0 < blanked < pos
    for o in (a, b):
        o.SetupBlanker(True, thresh, width, fs / 2)            # SampleRate==SampleRate: a rate-only change is ignored, state kept
    same(a.ProcessBlanker(x[pos:pos + 4000]), b.ProcessBlanker(x[pos:pos + 4000]), "after the ignored rate change")
    for o in (a, b):
        o.SetupBlanker(False, thresh, width, fs)
    same(a.ProcessBlanker(x[:100]), b.ProcessBlanker(x[:100]), "switched off")


def test_fir_iir_words(O, R):
    rng = np.random.default_rng(1)
    x = rng.standard_normal(3000) * 1000
    xc = x + 1j * rng.standard_normal(3000) * 1000
    for kind, args in (("lp", (1.0, 50.0, 5000, 9000, 31250.0)), ("hp", (1.0, 50.0, 5000, 3000, 62500.0)),
                       ("lp", (1.0, 40.0, 4500, 5500, 31250.0)), ("hp", (1.0, 50.0, 3000.0, 1800.0, 62500.0)),
                       ("lp", (2.5, 60.0, 10000, 18000, 62500.0))):
        a, b = O.CFir(), R.CFir()
        na = (a.InitLPFilter if kind == "lp" else a.InitHPFilter)(*args)
        nb = (b.InitLPFilter if kind == "lp" else b.InitHPFilter)(*args)
        assert na == nb
        if args[1] == 40.0:
            a.GenerateHBFilter(5000.0); b.GenerateHBFilter(5000.0)
        for ta, tb, name in zip(a.taps(), b.taps(), ("coef", "icoef", "qcoef")):
            same(ta, tb, (kind, args, name))
        for part in (slice(0, 1000), slice(1000, 3000)):
            same(a.ProcessFilter(x[part]), b.ProcessFilter(x[part]), (kind, args, "real"))
            same(a.ProcessFilter(xc[part]), b.ProcessFilter(xc[part]), (kind, args, "complex"))
    a, b = O.CFir(), R.CFir()
    a.InitConstFir([0.25, 0.5, 0.25]); b.InitConstFir([0.25, 0.5, 0.25])
    same(a.ProcessFilter(x), b.ProcessFilter(x), "const fir")
    for kind, f0, q, fs in (("LP", 3000.0, 1.0, 62500.0), ("HP", 300.0, 0.7, 31250.0), ("BP", 700.0, 5.0, 15625.0), ("BR", 25000, 1000.0, 100000)):
        a, b = O.CIir(), R.CIir()
        a.Init(kind, f0, q, fs); b.Init(kind, f0, q, fs)
        same(a.coefs(), b.coefs(), (kind, "coefficients"))
        same(a.ProcessFilter(x), b.ProcessFilter(x), (kind, "real"))
        same(a.ProcessFilter(xc), b.ProcessFilter(xc), (kind, "complex"))
        same(a.ProcessFilter(x[:7]), b.ProcessFilter(x[:7]), (kind, "real, state kept"))


@pytest.mark.parametrize("hang,slope,thresh,decay", [(0, 0, -100, 200), (1, 5, -60, 500), (0, 10, -20, 50)])
def test_agc_words(O, R, hang, slope, thresh, decay):
    """the parameter sets of test_agc_complex_and_real, both overloads, the hang timer, manual gain, and a
    SetParameters with a new sample rate in mid-stream (the rings are cleared)"""
    fs = 62500.0
    x = level_steps(62500, fs, 3)
    a, b = O.CAgc(), R.CAgc()
    for o in (a, b):
        o.SetParameters(True, bool(hang), thresh, 30, slope, decay, fs)
    for part in (slice(0, 8192), slice(8192, 40000), slice(40000, 40001), slice(40001, 62500)):
        same(a.ProcessData(x[part]), b.ProcessData(x[part]), ("agc complex", part))
    a2, b2 = O.CAgc(), R.CAgc()
    for o in (a2, b2):
        o.SetParameters(True, bool(hang), thresh, 30, slope, decay, fs)
    same(a2.ProcessData(x.real.copy()), b2.ProcessData(x.real.copy()), "agc real")
    for o in (a2, b2):
        o.SetParameters(False, bool(hang), thresh, 45, slope, decay, fs)
    same(a2.ProcessData(x[:1000]), b2.ProcessData(x[:1000]), "manual gain, complex")
    same(a2.ProcessData(x[:1000].real.copy()), b2.ProcessData(x[:1000].real.copy()), "manual gain, real")
    for o in (a, b):
        o.SetParameters(True, bool(hang), thresh, 30, slope, decay, 31250.0)
    same(a.ProcessData(x[:5000]), b.ProcessData(x[:5000]), "after a new sample rate")


def test_smeter_words(O, R):
    fs = 62500.0
    x = level_steps(40000, fs, 4)
    a, b = O.CSMeter(), R.CSMeter()
    for part in (slice(0, 8192), slice(8192, 40000)):
        a.ProcessData(x[part], fs); b.ProcessData(x[part], fs)
        assert a.GetAve() == b.GetAve()
    big = 40000.0 * np.exp(2j * np.pi * 0.01 * np.arange(500))
    a.ProcessData(big, fs); b.ProcessData(big, fs)
    assert a.GetPeak() == b.GetPeak() > 5.0
    assert a.GetPeak() == b.GetPeak() == 5.0                    # reset on read
    a.ProcessData(x[:100], 31250.0); b.ProcessData(x[:100], 31250.0)      # a new rate: the constants follow
    assert a.GetAve() == b.GetAve() and a.GetPeak() == b.GetPeak()


def test_leaf_demodulator_words(O, R):
    """AM, SAM, FM and SSB leaves on identical input, both overloads, whole and ragged calls; squelch decisions"""
    L, fs = 1024, 31250.0
    x = am_carrier(8 * L, fs, 150.0, fmod=800.0, depth=0.6, dbfs=-12.0)
    cuts = np.cumsum([0, 1, 17, 1000, 1025, 2500, 1, 4099, 333, 2048])
    xr = am_carrier(int(cuts[-1]), fs, 120.0, fmod=600.0, depth=0.5, dbfs=-10.0)
    for stereo in (False, True):
        a, b = O.CAmDemod(fs), R.CAmDemod(fs)
        a.SetBandwidth(4000.0); b.SetBandwidth(4000.0)
        sa, sb = O.CSamDemod(fs), R.CSamDemod(fs)
        for i in range(8):
            same(a.ProcessData(x[i * L:(i + 1) * L], stereo), b.ProcessData(x[i * L:(i + 1) * L], stereo), ("am", stereo, i))
            same(sa.ProcessData(x[i * L:(i + 1) * L], stereo), sb.ProcessData(x[i * L:(i + 1) * L], stereo), ("sam", stereo, i))
        for k in range(len(cuts) - 1):
            part = xr[cuts[k]:cuts[k + 1]]
            same(a.ProcessData(part, stereo), b.ProcessData(part, stereo), ("am ragged", stereo, k))
            same(sa.ProcessData(part, stereo), sb.ProcessData(part, stereo), ("sam ragged", stereo, k))
    fs = 62500.0
    x = fm_carrier(16 * L, fs, 300.0, fmod=1000.0, dev=3000.0, dbfs=-6.0, noise_dbfs=-60.0)
    xr = fm_carrier(int(cuts[-1]), fs, 300.0, fmod=1000.0, dev=3000.0, dbfs=-6.0, noise_dbfs=-60.0)
    rng = np.random.default_rng(5)
    noise = 3000.0 * (rng.standard_normal(8 * L) + 1j * rng.standard_normal(8 * L))
    for stereo in (False, True):
        a, b = O.CFmDemod(fs), R.CFmDemod(fs)
        a.SetSquelch(50); b.SetSquelch(50)
        for i in range(16):
            same(a.ProcessData(x[i * L:(i + 1) * L], 5000.0, stereo), b.ProcessData(x[i * L:(i + 1) * L], 5000.0, stereo), ("fm", stereo, i))
            assert a.squelched() == b.squelched(), i
        assert not b.squelched()
        for i in range(8):                                      # the carrier goes: the squelch shuts, same burst on both sides
            same(a.ProcessData(noise[i * L:(i + 1) * L], 5000.0, stereo), b.ProcessData(noise[i * L:(i + 1) * L], 5000.0, stereo), ("fm noise", i))
            assert a.squelched() == b.squelched(), i
        assert b.squelched()
        for k in range(len(cuts) - 1):
            part = xr[cuts[k]:cuts[k + 1]]
            same(a.ProcessData(part, 5000.0, stereo), b.ProcessData(part, 5000.0, stereo), ("fm ragged", stereo, k))
            assert a.squelched() == b.squelched(), k
    same(O.ssb_demod(x[:100]), R.ssb_demod(x[:100]), "ssb mono")
    same(O.ssb_demod(x[:100], True), R.ssb_demod(x[:100], True), "ssb stereo")


def test_pll_words_out_in_out_of_the_clamp(O, R):
    """the carriers of test_pll_unlockable_carrier_and_relock"""
    L, fs = 1024, 62500.0
    n = 12 * L
    t = np.arange(3 * n) / fs
    seg = lambda f, k: 8000.0 * np.exp(2j * np.pi * f * t[k * n:(k + 1) * n])
    for stereo in (False, True):
        x = np.concatenate([seg(9000.0, 0), seg(800.0, 1), seg(-11000.0, 2)])
        a, b = O.CFmDemod(fs), R.CFmDemod(fs)
        a.SetSquelch(50); b.SetSquelch(50)
        for i in range(3 * n // L):
            same(a.ProcessData(x[i * L:(i + 1) * L], 5000.0, stereo), b.ProcessData(x[i * L:(i + 1) * L], 5000.0, stereo), ("fm", stereo, i))
            assert a.squelched() == b.squelched(), i
    fs = 31250.0
    t = np.arange(3 * n) / fs
    for stereo in (False, True):
        x = np.concatenate([seg(3000.0, 0), seg(200.0, 1), seg(-2500.0, 2)]) * (1.0 + 0.3 * np.sin(2 * np.pi * 700.0 * t))
        a, b = O.CSamDemod(fs), R.CSamDemod(fs)
        for i in range(3 * n // L):
            same(a.ProcessData(x[i * L:(i + 1) * L], stereo), b.ProcessData(x[i * L:(i + 1) * L], stereo), ("sam", stereo, i))


# ------------------------------------------------------------------------------------------------ FFT stages
def test_fastfir_2048(O, R):
    """ragged calls through the 2048-point filter, four pass bands; the response H[k] as well"""
    fs = 62500.0
    cuts = (1, 1023, 1024, 2500, 333, 4096, 3600)
    x = tones_plus_noise(4, sum(cuts), fs, [1000.0, -3000.0, 20000.0])
    worst = worst_h = 0.0
    for lo, hi, off in [(-5000, 5000, 0), (100, 2800, 0), (-2800, -100, 0), (-250, 250, 700)]:
        a, b = O.CFastFIR(2048), R.CFastFIR(2048)
        a.SetupParameters(lo, hi, off, fs); b.SetupParameters(lo, hi, off, fs)
        ha, hb = a.coef(), b.coef()
        worst_h = max(worst_h, np.abs(ha - hb).max() / np.abs(hb).max())
        # H = Fwd(h): unscaled transform of taps whose largest is max|h|; max|H| <= sum|h|, so in units of max|H| the
        # bound FFT_EPS * N * max|h| is at most FFT_EPS * N
        assert np.abs(ha - hb).max() <= FFT_EPS * 2048 * np.abs(np.fft.fft(hb)).max() / 2048
        pos = 0
        for n in cuts:
            ya, yb = a.ProcessData(x[pos:pos + n]), b.ProcessData(x[pos:pos + n]); pos += n
            assert len(ya) == len(yb)
            if len(yb):
                worst = max(worst, np.abs(ya - yb).max() / np.abs(x).max())
        assert pos == len(x)
    fig("CFastFIR 2048, max|err| / max|x|", worst); fig("CFastFIR response, max|err| / max|H|", worst_h)
    assert worst <= FFT_EPS


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192, 16384, 32768, 65536])
def test_plain_transforms(O, R, n):
    rng = np.random.default_rng(n)
    x = 1000 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    f = R.CFft(); f.SetFFTParams(n, False, 0.0, 1.0)
    ef = np.abs(f.FwdFFT(x) - O.fft(x, +1)).max() / (n * np.abs(x).max())
    er = np.abs(f.RevFFT(x) - O.fft(x, -1)).max() / (n * np.abs(x).max())
    fig("FwdFFT %d, max|err| / (N max|x|)" % n, ef); fig("RevFFT %d" % n, er)
    assert ef <= FFT_EPS and er <= FFT_EPS
    same(R.fft(x, +1), f.FwdFFT(x), "module-level fft is FwdFFT")


@pytest.mark.parametrize("n,ave", [(512, 2), (2048, 4), (4096, 1), (65536, 1)])
def test_display_spectrum(O, R, n, ave):
    """5 frames; the bels compared in the linear domain: 10^(bel - K_B) = averaged power + K_C (fft.cpp:186-188, 555-570),
    and a transform error of e = FFT_EPS * N * max|window * x| per bin moves a power P by at most 2 sqrt(P) e + e^2
    (the average is a convex combination, Cauchy-Schwarz); 1e-13 P on top for log10 and pow (37 = 16 bels * ln 10
    times their half-ulp errors).  Pixels equal at heights 300 and 65536, overload flag and return values equal."""
    fs = 2e6
    a, b = O.CFft(), R.CFft()
    for o in (a, b):
        o.SetFFTParams(n, False, 0.0, fs); o.SetFFTAve(ave)
    kb = -2.0 * np.log10(n * O.constants()["fft.cpp:K_AMPMAX"] / 2.0)
    worst = 0.0
    for k in range(5):
        x = tones_plus_noise(k, n, fs, [250e3, -611e3 + 977.0 * k], start=k * n)
        assert a.PutInDisplayFFT(x) == b.PutInDisplayFFT(x) == k + 1
        pa, pb = 10.0 ** (a.ave_buf() - kb), 10.0 ** (b.ave_buf() - kb)
        e = FFT_EPS * n * 2.0 * np.abs(x).max()
        room = 2.0 * np.sqrt(pb) * e + e * e + 1e-13 * pb
        worst = max(worst, (np.abs(pa - pb) / room).max())
        assert (np.abs(pa - pb) <= room).all(), (n, k)
        for h, w, lo, hi, mindb in ((1 << 16, min(700, n // 2), -900000, 900000, -160.0), (300, min(n - 1, 30000), -1000000, 1000000, -220.0)):
            (ova, pxa), (ovb, pxb) = a.GetScreenIntegerFFTData(h, w, 0.0, mindb, lo, hi), b.GetScreenIntegerFFTData(h, w, 0.0, mindb, lo, hi)
            assert ova == ovb is False
            same(pxa, pxb, ("pixels", n, k, h))
    fig("display %d, worst power difference / allowed" % n, worst)
    big = x.copy(); big[5] = 32500.0
    assert a.PutInDisplayFFT(big) == b.PutInDisplayFFT(big)
    (ova, pxa), (ovb, pxb) = a.GetScreenIntegerFFTData(100, 50, 0.0, -100.0, 0, 500000), b.GetScreenIntegerFFTData(100, 50, 0.0, -100.0, 0, 500000)
    assert ova is True and ovb is True
    same(pxa, pxb, "pixels of the overloaded frame")
    a.SetFFTAve(1); b.SetFFTAve(1)                               # resets counts and sums
    assert a.PutInDisplayFFT(x) == b.PutInDisplayFFT(x) == 1
    a.SetFFTParams(n, True, 0.0, fs); b.SetFFTParams(n, True, 0.0, fs)      # inverted spectrum
    a.PutInDisplayFFT(x); b.PutInDisplayFFT(x)
    same(a.GetScreenIntegerFFTData(300, 200, 0.0, -160.0, -500000, 700000)[1], b.GetScreenIntegerFFTData(300, 200, 0.0, -160.0, -500000, 700000)[1], "inverted")


# ------------------------------------------------------------------------------------------------ the whole CDemodulator
def _pair(O, R, mode, fs, freq=-100e3):
    m, kw = MODES[mode]
    a, b = O.CDemodulator(2048), R.CDemodulator(2048)
    a.enable_taps(True)
    for o, mod in ((a, O), (b, R)):
        o.SetInputSampleRate(fs); o.SetDemod(m, info(mod, **kw)); o.SetDemodFreq(freq)
    assert a.GetOutputRate() == b.GetOutputRate() and a.buf_limit() == b.buf_limit()
    return a, b


def _taps_equal(a, b, R, before, stereo=False):
    """the reference's recorded DisplayData calls of one ProcessData call against what the oracle's taps grew by:
    profile order 1, 2, 3, 4 per pass, lengths, rates; the first value of every PROFILE_1 buffer (no FFT in front of
    it) word for word"""
    calls = R.tap_calls()
    R.clear_tap_calls()
    assert [c[0] for c in calls] == [1, 2, 3, 4] * (len(calls) // 4)
    assert all(c[3] == b.GetOutputRate() for c in calls)
    now = [len(a.tap(k)) * (2 if k < 4 else 1) for k in (1, 2, 3, 4)]          # in doubles
    for k in (1, 2, 3, 4):
        assert all(c[2] == (k < 4 or stereo) for c in calls if c[0] == k), ("tap", k)
        assert sum(c[1] * (2 if c[2] else 1) for c in calls if c[0] == k) == now[k - 1] - before[k - 1], ("tap", k)
    t1 = a.tap(1)
    pos = before[0] // 2
    for c in calls:
        if c[0] == 1 and c[1]:
            assert t1[pos].real == c[4], "PROFILE_1 first value"
            pos += c[1]
    return now


def check_bursts(errs, mode, what, stereo=False, fm_from=14):
    """the rule of the module docstring on per-burst errors from the stream's first burst"""
    e = np.asarray(errs, dtype=float) / FULL_SCALE
    fig("%s %s per-burst max, of full scale: first %s ... last %.2g" % (what, mode, ["%.2g" % v for v in e[:6]], e[-1] if len(e) else 0.0), e.max() if len(e) else 0.0)
    assert np.isfinite(e).all()
    if mode == "FM":
        big = np.flatnonzero(e[:3] > 0.2)
        start = int(big[0]) if len(big) else 0
        assert (e <= 2.5).all()
        for k in range(1, len(SB.FM_STARTUP)):
            assert (e[start + k:] <= SB.FM_STARTUP[k]).all(), (what, k, e[:8])
        crossed = int(np.flatnonzero(e > 1e-9)[-1]) + 1 if (e > 1e-9).any() else 0
        fig("%s FM: first burst from which every burst is <= 1e-9 of full scale" % what, crossed)
        assert len(e) > fm_from and (e[fm_from:] <= 1e-9).all(), (what, crossed, e[fm_from:])
    elif mode == "SAM":
        assert e[0] <= SB.SAM_FIRST and e[1] <= SB.SAM_SECOND, (what, e[:3])
        assert len(e) > 2 and (e[2:] <= 1e-9).all(), (what, e[:6])
    else:
        assert len(e) and (e <= 1e-9).all(), (what, e[:6])


N_SAMPLES = {"FM": 21 * 32768, "USB": 10 * 32768, "LSB": 10 * 32768, "AM": 9 * 65536, "SAM": 9 * 65536, "CWU": 6 * 131072, "CWL": 6 * 131072}


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
@pytest.mark.parametrize("mode", ["AM", "SAM", "FM", "USB", "LSB", "CWU", "CWL"])
def test_chain_reference_call_pattern(O, R, mode, stereo):
    """2 MS/s, calls of 256 x 13 samples (uneven against the 19968-sample window), both overloads of ProcessData"""
    fs = 2e6
    a, b = _pair(O, R, mode, fs)
    R.clear_tap_calls()
    x = chain_input(mode, N_SAMPLES[mode], fs)
    errs, taps = [], [0, 0, 0, 0]
    for i in range(0, len(x), 256 * 13):
        ka, oa = a.ProcessData(x[i:i + 256 * 13], stereo)
        kb, ob = b.ProcessData(x[i:i + 256 * 13], stereo)
        assert ka == kb
        taps = _taps_equal(a, b, R, taps, stereo)
        if kb:
            assert kb == 1024
            errs.append(np.abs(oa[:kb] - ob[:kb]).max())
            if mode == "FM":
                assert (not oa[:kb].any()) == (not ob[:kb].any())
            assert not oa[kb:].any() and not ob[kb:].any()
    check_bursts(errs, mode, "2 MS/s %s" % ("stereo" if stereo else "mono"), stereo)
    assert abs(a.GetSMeterAve() - b.GetSMeterAve()) <= SMETER_EPS and abs(a.GetSMeterPeak() - b.GetSMeterPeak()) <= SMETER_EPS
    fig("S-meter difference, dB", abs(a.GetSMeterAve() - b.GetSMeterAve()))


def test_chain_fm_at_10_msps(O, R):
    """10 MS/s -> 78125 S/s: the first burst is silent on both sides, the pull-in is burst 1, and the start-up difference
    decays by 3.7 per burst (startup_bounds.py): 0.064 * 3.7^-k <= 1e-9 from k = 14, so burst 15; asserted from 18"""
    fs = 10e6
    a, b = _pair(O, R, "FM", fs, freq=-1.2e6)
    assert a.GetOutputRate() == 78125.0
    x = fm_carrier(a.buf_limit() * 32, fs, 1.2e6, fmod=1000.0, dev=3000.0, dbfs=-20.0)
    ga, gb = a.process_append(x), b.process_append(x)
    assert len(ga) == len(gb) >= 22 * 1024
    check_bursts(burst_errors(ga, gb), "FM", "10 MS/s", fm_from=18)


def test_overwrite_at_out0_return_convention(O, R):
    """a call that holds several passes returns the SUM of their counts with only the last pass's audio at out[0]"""
    a, b = _pair(O, R, "USB", 2e6)
    x = chain_input("USB", 19968 * 8, 2e6)
    a.ProcessData(x[:19968 * 4]); b.ProcessData(x[:19968 * 4])
    ka, oa = a.ProcessData(x[19968 * 4:], out_cap=8192)
    kb, ob = b.ProcessData(x[19968 * 4:], out_cap=8192)
    assert ka == kb == 2048                                       # 2496 decimated samples on 1408 kept: two bursts
    assert np.abs(oa - ob).max() <= CHAIN_EPS and ob[:1024].any() and not ob[1024:].any() and not oa[1024:].any()


def test_cw_offset_double_add_through_set_demod_freq(O, R):
    """SetDemodFreq hands m_CW_Offset to the down-converter and SetFrequency adds it; every SetDataRate adds it once
    more (downconvert.cpp:169)"""
    m, kw = MODES["CWU"]
    b = R.CDemodulator(2048)
    od = O.CDownConvert()
    b.SetInputSampleRate(2e6); od.SetDataRate(2e6, 48000.0)
    assert b.nco_freq() == od.nco_freq() == 0.0
    b.SetDemod(m, info(R, **kw)); od.SetDataRate(2e6, 1000.0); od.SetCwOffset(700.0)
    b.SetDemodFreq(-100e3); od.SetFrequency(-100e3)
    assert b.nco_freq() == od.nco_freq() == -100e3 + 700.0
    b.SetInputSampleRate(500e3); od.SetDataRate(500e3, 1000.0)
    assert b.nco_freq() == od.nco_freq() == -100e3 + 1400.0
    assert b.stages() == od.stages()


def _feed(a, b, x, call):
    ga, gb = [], []
    for i in range(0, len(x), call):
        ya, yb = a.process_append(x[i:i + call]), b.process_append(x[i:i + call])
        assert len(ya) == len(yb)
        ga.append(ya); gb.append(yb)
    return np.concatenate(ga), np.concatenate(gb)


def _steady(ga, gb, mode, what, settle=0):
    """a segment behind a control call in mid-stream: both sides made the same change at the same sample, so the
    steady bound holds on from `settle` bursts behind it (a PLL that was restarted gets the start-up rule instead)"""
    e = burst_errors(ga[:len(ga) // 1024 * 1024], gb[:len(gb) // 1024 * 1024]) / FULL_SCALE
    fig("%s %s: worst burst behind burst %d, of full scale (first %s)" % (what, mode, settle, ["%.2g" % v for v in e[:4]]), e[settle:].max())
    assert np.isfinite(e).all() and (e <= 2.5).all()
    assert (e[settle:] <= 1e-9).all(), (what, mode, e[:8])


@pytest.mark.parametrize("new_rate", [500e3, RADIO_RATE], ids=["500k", "615k"])
@pytest.mark.parametrize("mode", ["FM", "AM", "USB", "CWU", "SAM"])
def test_input_rate_change_in_mid_stream(O, R, mode, new_rate):
    """the sequence of tests/test_rate_change_gpu.py::test_dropin_input_rate_change_in_mid_stream: SetInputSampleRate with
    a partly filled window and NO SetDemod (filter, AGC, window and demodulator stay stale), then SetDemod with the same
    mode, then back.  Every count, rate and window length equal; the audio under the steady bound as soon as the
    stream's own start-up (FM 14 bursts, SAM 2) is over -- nothing a control call does may separate the two."""
    from test_rate_change_gpu import _signal
    a, b = _pair(O, R, mode, 2e6)
    m, kw = MODES[mode]
    lim = a.buf_limit()
    ga, gb = _feed(a, b, _signal(mode, 80 * 5000 + (14 * 32768 if mode == "FM" else 0), 2e6), 5000)
    check_bursts(burst_errors(ga[:len(ga) // 1024 * 1024], gb[:len(gb) // 1024 * 1024]), mode, "before the change", fm_from=14)
    assert a.buf_limit() == b.buf_limit() and b.buf_pos() > 0
    a.SetInputSampleRate(new_rate); b.SetInputSampleRate(new_rate)
    assert a.GetOutputRate() == b.GetOutputRate() and a.buf_limit() == b.buf_limit() == lim
    ga, gb = _feed(a, b, _signal(mode, 24 * lim + 3000, new_rate), 7000)
    assert len(gb) >= 3 * 1024
    _steady(ga, gb, mode, "after SetInputSampleRate")
    assert abs(a.GetSMeterAve() - b.GetSMeterAve()) <= SMETER_EPS
    a.SetDemod(m, info(O, **kw)); b.SetDemod(m, info(R, **kw))
    assert a.buf_limit() == b.buf_limit() != lim and a.GetOutputRate() == b.GetOutputRate()
    ga, gb = _feed(a, b, _signal(mode, 120 * a.buf_limit(), new_rate), 9000)
    _steady(ga, gb, mode, "after SetDemod at the new rate")
    a.SetInputSampleRate(2e6); b.SetInputSampleRate(2e6)
    a.SetDemod(m, info(O, **kw)); b.SetDemod(m, info(R, **kw))
    assert a.buf_limit() == b.buf_limit() == lim
    ga, gb = _feed(a, b, _signal(mode, 30 * lim, 2e6), lim)
    _steady(ga, gb, mode, "back at 2 MS/s")
    assert abs(a.GetSMeterAve() - b.GetSMeterAve()) <= SMETER_EPS


def test_same_mode_set_demod_and_mode_changes_in_mid_stream(O, R):
    """USB with new edges (same mode: the demodulator object stays), USB -> AM -> FM -> CWU (new objects, new plans);
    every segment in calls that do not end on a window"""
    fs = 2e6
    a, b = _pair(O, R, "USB", fs)
    x = chain_input("USB", 12 * 32768, fs)
    ga, gb = _feed(a, b, x, 7000)
    _steady(ga, gb, "USB", "start")
    kw = dict(MODES["USB"][1], HiCut=2400, LowCut=300, AgcDecay=500, AgcSlope=5)
    a.SetDemod(3, info(O, **kw)); b.SetDemod(3, info(R, **kw))
    ga, gb = _feed(a, b, x, 7000)
    _steady(ga, gb, "USB", "new edges, same mode")
    for mode, n in (("AM", 9 * 65536), ("FM", 21 * 32768), ("CWU", 6 * 131072)):
        m, kw = MODES[mode]
        a.SetDemod(m, info(O, **kw)); b.SetDemod(m, info(R, **kw))
        assert a.GetOutputRate() == b.GetOutputRate() and a.buf_limit() == b.buf_limit()
        ga, gb = _feed(a, b, chain_input(mode, n, fs), 9000)
        errs = burst_errors(ga[:len(ga) // 1024 * 1024], gb[:len(gb) // 1024 * 1024])
        check_bursts(errs, mode, "after the change to")
    assert abs(a.GetSMeterAve() - b.GetSMeterAve()) <= SMETER_EPS
