"""The reference-derived known answers of tests/golden/survey_anchors.json (SURVEY.md section 8c /
App. A.9) replayed directly against the HIP path through the C ABI -- no oracle in between.
Tolerances are the fixture's own, widened only where fp32 device arithmetic needs it (stated)."""
import json
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "survey_anchors.json")))


def test_nco_envelope():
    import cutesdr_amd as ca
    g = GOLDEN["nco_envelope"]
    dc = ca.CDownConvert()
    dc.SetDataRate(g["input"]["in_rate"], g["input"]["max_bw"])
    assert dc.stages() == []
    dc.SetFrequency(g["input"]["nco_hz"])
    mag = np.abs(dc.ProcessData(np.ones(2000, dtype=np.complex128)))
    e = g["expect"]
    tol = 2e-6                                               # fp32 phasor and amplitude table
    assert mag[0] == pytest.approx(e["mag_0"], abs=tol)
    assert mag[1] == pytest.approx(e["mag_1"], abs=tol)
    assert mag[10] == pytest.approx(e["mag_10"], abs=tol)
    assert mag[-1] == pytest.approx(e["mag_inf"], abs=tol)


def test_cw_offset_double_add_and_chains():
    import cutesdr_amd as ca
    g = GOLDEN["cw_offset_double_add"]
    dc = ca.CDownConvert()
    dc.SetCwOffset(g["input"]["cw_offset"])
    dc.SetFrequency(g["input"]["frequency"])
    assert dc.nco_freq() == g["expect"]["nco_after_set_frequency"]
    assert dc.SetDataRate(g["input"]["in_rate"], g["input"]["max_bw"]) == g["expect"]["out_rate"]
    assert dc.nco_freq() == g["expect"]["nco_after_set_data_rate"]
    assert dc.stages() == g["expect"]["stages"]
    for c in GOLDEN["decimator_chains"]["cases"]:
        d = ca.CDownConvert()
        assert d.SetDataRate(c["in_rate"], c["max_bw"]) == c["out_rate"]
        assert d.stages() == c["stages"]


def test_resampler_delay_and_count():
    import cutesdr_amd as ca
    e = GOLDEN["resampler"]["expect"]
    rng = np.random.default_rng(5)
    x = rng.standard_normal(e["in_count"])
    r = ca.CFractResampler(); r.Init(8192)
    y = r.Resample(x, 1.0)
    assert len(y) == e["in_count"]
    d = e["unity_rate_delay"]
    np.testing.assert_allclose(y[d:], x[:-d], atol=1e-5 * np.abs(x).max())    # fp32 table and samples
    r2 = ca.CFractResampler(); r2.Init(8192)
    assert len(r2.Resample(x, e["rate"])) == e["out_count"]


def test_display_peak():
    import cutesdr_amd as ca
    g = GOLDEN["display_fft_c1"]
    i, e = g["input"], g["expect"]
    f = ca.CFft(); f.SetFFTParams(i["n"], False, i["db_comp"], i["fs"]); f.SetFFTAve(i["ave"])
    f.PutInDisplayFFT(i["tone_amplitude"] * np.exp(2j * np.pi * i["tone_hz"] * np.arange(i["n"]) / i["fs"]))
    a = f.ave_buf()
    assert np.argmax(a) == e["peak_index"]
    assert a[e["peak_index"]] == pytest.approx(e["peak_bels"], abs=e["tol_bels"])


def test_fm_chain_rate_limit_and_smeter():
    import cutesdr_amd as ca
    g = GOLDEN["fm_chain"]
    i, e = g["input"], g["expect"]
    d = ca.CDemodulator(i["fastfir_n"])
    d.SetInputSampleRate(i["in_rate"])
    d.SetDemod(ca.DEMOD_FM, ca.fm_defaults())
    d.SetDemodFreq(i["demod_freq"])
    assert d.GetOutputRate() == e["out_rate"]
    assert d.buf_limit() == e["in_buf_limit"]
    n = i["samples"]
    x = i["carrier_amplitude"] * np.exp(2j * np.pi * i["carrier_hz"] * np.arange(n) / i["in_rate"])
    for k in range(0, n, 1 << 16):
        d.ProcessData(x[k:k + (1 << 16)])
    assert d.GetSMeterAve() == pytest.approx(e["smeter_ave_db"], abs=e["tol_db"])


def test_fastfir_16384_delay():
    import cutesdr_amd as ca
    g = GOLDEN["fastfir_16384"]
    i, e = g["input"], g["expect"]
    n, fs = i["n"], i["fs"]
    ff = ca.CFastFIR(n)
    ff.SetupParameters(i["lo_cut"], i["hi_cut"], 0, fs)
    t = np.arange(n * 6)
    x = np.exp(2j * np.pi * i["pass_tone_hz"] * t / fs) + np.exp(2j * np.pi * i["stop_tone_hz"] * t / fs)
    y = ff.ProcessData(x)
    assert len(y) == (len(x) // (n // 2)) * (n // 2)
    want = np.exp(2j * np.pi * i["pass_tone_hz"] * (t[:len(y)] - e["delay_samples"]) / fs)
    assert np.abs(y[n:] - want[n:]).max() < e["max_err"]


# ---- tests/golden/reference_vectors.json: outputs of the reference's own compiled code, replayed on the HIP path ----
def _reference_vectors():
    import importlib.util
    here = os.path.dirname(__file__)
    spec = importlib.util.spec_from_file_location("make_reference_vectors", os.path.join(here, "golden", "make_reference_vectors.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod, json.load(open(os.path.join(here, "golden", "reference_vectors.json")))


RV, VECTORS = _reference_vectors()


@pytest.mark.parametrize("name", sorted(VECTORS))
def test_reference_vectors_on_the_hip_path(name):
    """Every recorded case through the library's drop-in classes, each under the tolerance its stage has in the parity
    tests (named per kind below); counts exact.  The words compared are the stored first and last 32; where one
    tolerance holds for every word the three digests are held to n times it."""
    import cutesdr_amd as ca
    import dc_ref as D
    import test_postchain_gpu as TP
    FS = 32767.0
    case = VECTORS[name]
    e, kind = case["expect"], case["kind"]
    v = RV.run_case(ca, case)
    first = np.array([float.fromhex(h) for h in e["first"]]); last = np.array([float.fromhex(h) for h in e["last"]])
    assert len(v) == e["n"]
    gf, gl = v[:RV.WORDS], v[-RV.WORDS:]
    x = RV.make_input(case)
    if kind in ("ssb", "blanker"):                               # copies and zeros of fp32-representable input: exact
        assert np.array_equal(gf, first) and np.array_equal(gl, last)
        tol = 0.0
    elif kind == "display":                                      # test_fft_resampler_gpu.assert_spectrum_close, word by word
        for got, want in ((gf, first), (gl, last)):
            lim = np.where(want > e["max"] - 6.0, 0.001, np.where(want > e["max"] - 9.0, 0.05, 0.2))
            assert (np.abs(got - want) <= lim)[want > -15.0].all()
        assert int(np.argmax(v)) == 2560 and abs(v.max() - e["max"]) <= 0.001
        return
    elif kind == "chain":                                        # test_postchain_gpu: the chain rule
        mode = case["params"]["mode"]
        if mode == "FM":
            assert e["n"] >= 7 * 1024 and np.abs(gl - last).max() <= TP.FM_STEADY and np.abs(gf - first).max() <= 2.5 * FS
        else:
            assert e["n"] >= 3 * 1024 and np.abs(gf - first).max() <= TP.FROM_ZERO and np.abs(gl - last).max() <= TP.STEADY
        return
    else:
        tol = {"downconvert": D.K * np.sqrt(2.0) * e["rms"],               # test_downconvert_plans_gpu.assert_parity
               "fastfir": 2e-5 * np.abs(x).max(),                          # test_fastfir_gpu
               "fft": 2e-5 * len(x) * np.abs(x).max() / np.sqrt(len(x)) * 4,   # test_fft_resampler_gpu.test_plain_transforms
               "fir": 2e-3, "iir": 5e-3,                                   # test_postchain_gpu, the leaf filters
               "agc": TP.STEADY, "am": TP.STEADY, "sam": TP.STEADY, "fm": TP.STEADY,
               "smeter": 0.01, "resampler": 1e-5 * 8000 * 6}[kind]
        skip = 2 if kind == "downconvert" else 0                            # assert_parity leaves out the first sample
        assert np.abs(gf - first)[skip:].max() <= tol and np.abs(gl - last).max() <= tol, (np.abs(gf - first).max(), np.abs(gl - last).max(), tol)
        if skip:
            return
    d = RV.digest(v)
    assert all(abs(d[k] - e[k]) <= e["n"] * tol for k in ("sum", "abs", "dot")), (d, e, tol)
