"""CPU tests of the product's HOST-side setup logic (no GPU): filter design, decimator stage
selection, NCO bookkeeping and the spectrum-order map of the FFT kernel, checked against the
oracle and against an independent numpy statement of the kernel's index algebra."""
import ctypes as C
import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_fastfir_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.csdr__host_fastfir_bin_of.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.csdr__host_dc_plan.argtypes = [C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.csdr__host_dc_stage_taps.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.csdr__host_dc_nco.argtypes = [C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.csdr__host_dc_nco.restype = None
    lib.csdr__host_fir_design.argtypes = [C.c_int] + [C.c_double] * 6 + [C.c_void_p] * 3
    lib.csdr__host_iir_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p]
    lib.csdr__host_iir_design.restype = None
    lib.csdr__host_agc_params.argtypes = [C.c_int] * 6 + [C.c_double, C.c_void_p]
    lib.csdr__host_agc_params.restype = None
    return lib


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n", [2048, 16384])
@pytest.mark.parametrize("cuts", [(-5000, 5000, 0), (100, 2800, 0), (-2800, -100, 0), (-250, 250, 700)])
def test_fastfir_response_matches_oracle(L, oracle, n, cuts):
    H = np.zeros(n, dtype=np.complex128)
    assert L.csdr__host_fastfir_design(n, cuts[0], cuts[1], cuts[2], 62500.0, vp(H)) == 0
    ff = oracle.CFastFIR(n)
    assert ff.SetupParameters(cuts[0], cuts[1], cuts[2], 62500.0) == 1
    np.testing.assert_allclose(H, ff.coef(), atol=1e-13)


def test_fastfir_rejects_like_reference(L, oracle):
    H = np.zeros(2048, dtype=np.complex128)
    for lo, hi in ((5000, -5000), (-40000, 100), (100, 31250)):
        assert L.csdr__host_fastfir_design(2048, lo, hi, 0, 62500.0, vp(H)) == -1
        assert oracle.CFastFIR(2048).SetupParameters(lo, hi, 0, 62500.0) == -1


@pytest.mark.parametrize("log2n", [11, 12, 13, 14])
def test_spectrum_order_is_a_permutation_and_matches_index_algebra(L, log2n):
    n = 1 << log2n
    r0 = n // 1024
    seen = np.zeros(n, dtype=bool)
    for t in range(n // 32):
        for r in range(32):
            k = L.csdr__host_fastfir_bin_of(log2n, t, r)
            k2 = int("{:05b}".format(r)[::-1], 2)
            assert k == (t >> 5) + r0 * ((t & 31) + 32 * k2)
            seen[k] = True
    assert seen.all()


@pytest.mark.parametrize("in_rate,bw", [(2e6, 15000), (2e6, 10000), (2e6, 20000), (2e6, 1000), (10e6, 15000),
                                        (615385.0, 3000), (48000.0, 20000), (100000.0, 10000), (8e6, 500)])
def test_decimator_plan_matches_oracle(L, oracle, in_rate, bw):
    codes = np.zeros(16, dtype=np.int32)
    rate = C.c_double(); W = C.c_int()
    n = L.csdr__host_dc_plan(in_rate, bw, vp(codes), C.byref(rate), C.byref(W))
    dc = oracle.CDownConvert()
    if (in_rate, bw) == (100000.0, 10000):
        dc.SetDataRate(1.0, 1.0)          # the constructor already holds these values: force a rebuild
    assert dc.SetDataRate(in_rate, bw) == rate.value
    assert dc.stages() == list(codes[:n])
    need = sum((2 if c == 3 else c - 1) << s for s, c in enumerate(codes[:n]))
    assert W.value >= need and W.value % (1 << n) == 0 if n else W.value == 0


def test_decimator_taps_match_tables(L):
    import re, os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "csdr_hb_taps.h")).read()
    h = np.zeros(64)
    Ln = L.csdr__host_dc_stage_taps(2e6, 15000.0, 4, vp(h))            # HB31 of the FM chain
    assert Ln == 31
    ev = [float(v) for v in re.search(r"/\* HB31 \*/ \{([^}]*)\}", hdr).group(1).split(",")][:8]
    want = np.zeros(31); want[0:15:2] = ev; want[15] = 0.5; want[16:31:2] = ev[::-1]
    np.testing.assert_allclose(h[:31], want, rtol=1e-7)
    assert L.csdr__host_dc_stage_taps(2e6, 1000.0, 0, vp(h)) == 4      # CIC3 as 4 taps
    np.testing.assert_allclose(h[:4], [0.125, 0.375, 0.375, 0.125])


def test_nco_increment_and_cw_offset(L):
    inc = C.c_ulonglong(); stored = C.c_double()
    L.csdr__host_dc_nco(1000.0, 700.0, 2e6, C.byref(inc), C.byref(stored))
    assert stored.value == 1700.0
    assert inc.value / 2.0 ** 64 == pytest.approx(1700.0 / 2e6, rel=1e-15)
    L.csdr__host_dc_nco(-250e3, 0.0, 2e6, C.byref(inc), C.byref(stored))
    assert inc.value / 2.0 ** 64 == pytest.approx(1.0 - 0.125, rel=1e-15)   # negative frequency wraps


@pytest.mark.parametrize("kind,args,hb", [(0, (1.0, 50.0, 5000.0, 9000.0, 31250.0), 0.0),
                                          (0, (1.0, 40.0, 4500.0, 5500.0, 31250.0), 5000.0),
                                          (1, (1.0, 50.0, 5000.0, 3000.0, 62500.0), 0.0),
                                          (0, (1.0, 50.0, 10000.0, 18000.0, 62500.0), 0.0)])
def test_kaiser_fir_design_matches_oracle(L, oracle, kind, args, hb):
    c = np.zeros(80); i = np.zeros(80); q = np.zeros(80)
    n = L.csdr__host_fir_design(kind, *args, hb, vp(c), vp(i), vp(q))
    r = oracle.CFir()
    n2 = (r.InitLPFilter if kind == 0 else r.InitHPFilter)(*args)
    if hb:
        r.GenerateHBFilter(hb)
    assert n == n2
    for a, b in zip((c, i, q), r.taps()):
        np.testing.assert_allclose(a[:n], b, atol=1e-15)


def test_biquad_and_agc_parameters_match_oracle(L, oracle):
    c5 = np.zeros(5)
    for kind, name in enumerate(("LP", "HP", "BP", "BR")):
        L.csdr__host_iir_design(kind, 3000.0, 1.0, 62500.0, vp(c5))
        r = oracle.CIir(); r.Init(name, 3000.0, 1.0, 62500.0)
        np.testing.assert_allclose(c5, r.coefs(), rtol=1e-15)
    # RBJ cookbook cross-check of the low-pass (published algorithm)
    w0 = 2 * np.pi * 3000.0 / 62500.0; al = np.sin(w0) / 2.0
    L.csdr__host_iir_design(0, 3000.0, 1.0, 62500.0, vp(c5))
    np.testing.assert_allclose(c5, np.array([(1 - np.cos(w0)) / 2, 1 - np.cos(w0), (1 - np.cos(w0)) / 2,
                                             -2 * np.cos(w0), 1 - al]) / (1 + al), rtol=1e-14)
    p = np.zeros(12)
    L.csdr__host_agc_params(1, 0, -100, 30, 0, 200, 62500.0, vp(p))
    assert p[0] == -5.0 and p[1] == 0.0
    assert p[2] == pytest.approx(0.7 * 10 ** 5.0)
    assert (p[8], p[9], p[10]) == (937, 1125, 12500)
    assert p[4] == pytest.approx(1 - np.exp(-1 / (62500 * .002)))


def test_decimator_plan_enumeration_is_every_sequence_the_selection_rule_can_produce():
    """all_dc_plans() (cutesdr_amd/_build.py: the stage sequences a CSDR_ALL_DC_PLANS=1 build compiles the
    down-converter for) against a brute force over rates and bandwidths with the same selection rule: nothing the
    sweep finds is missing, every listed plan comes with a (rate, bandwidth) pair that selects it, and the default
    build's table (the reference's radio rates x demodulator bandwidths) is inside."""
    import importlib.util, os
    from cutesdr_amd import _build
    plans = _build.all_dc_plans()
    assert len(plans) == 164 and set(_build.DC_PLANS) <= set(plans)
    assert set(_build.default_dc_plans()) <= set(plans) and 20 <= len(_build.default_dc_plans()) <= 64
    for p, (rate, bw) in _build.DC_PLAN_PAIRS.items():
        assert _build.dc_plan(rate, bw) == p
    tables = _build._hb_tables()
    for p, (rate, bw) in plans.items():
        assert _build.dc_plan(rate, bw, tables) == p
        assert 1 <= len(p) <= 9 and all(k in (3, 11, 15, 19, 23, 27, 31, 35, 39, 43, 47, 51) for k in p)
        assert list(p) == sorted(p)
    swept = set()
    for ri in range(0, 700):
        rate = 16000.0 * 1.0105 ** ri
        for bi in range(0, 140):
            bw = 200.0 * 1.09 ** bi
            if bw > rate / 2: break
            q = _build.dc_plan(rate, bw, tables)
            if q: swept.add(q)
    assert swept <= set(plans) and len(swept) > 100
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("list_dc_plans", os.path.join(root, "tools", "list_dc_plans.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    assert set(m.table(m.RATES)) | set(m.table(m.MORE_RATES)) <= set(plans)


def test_the_retune_and_parameter_setters_hold_no_device_wide_synchronisation():
    """VERDICT r5 task 6, checked in the source: the functions behind set_freq, a same-mode SetDemod and the spectrum's
    readers contain no hipDeviceSynchronize (they queue patches -- csrc/patch_queue.hpp -- or wait on the object's own
    stream); the one exception is spelled out: CFastFIR's once-in-a-lifetime switch from a shared response to one per
    row reallocates.  (The GPU side: tests/test_control_plane_gpu.py.)"""
    import os, re
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cutesdr_amd", "csrc")

    def body(path, signature):
        txt = open(os.path.join(root, path)).read()
        i = txt.index(signature)
        j = txt.index("{", i)
        depth, k = 0, j
        while True:
            depth += txt[k] == "{"
            depth -= txt[k] == "}"
            k += 1
            if depth == 0:
                return txt[j:k]
    clean = [("capi_downconv.hip", "int csdr_downconvert_batch_set_frequency("), ("capi_downconv.hip", "int csdr_downconvert_batch_set_cw_offset("),
             ("capi_demod_batch.hip", "int csdr_demod_batch_set_freq("), ("capi_demod.hip", "int csdr_demod_set_freq("),
             ("pc_unit.hpp", "int agc_set("), ("pc_unit.hpp", "int smeter_rate_set("), ("pc_unit.hpp", "int fm_params_set("),
             ("pc_unit.hpp", "int am_bandwidth_set("), ("capi_fft.hip", "int csdr_fft_batch_get_ave("),
             ("capi_fft.hip", "int csdr_fft_batch_get_screen("), ("capi_fft.hip", "int csdr_fft_batch_get_total_count("),
             ("capi_fft.hip", "static int fft_read(")]
    for path, sig in clean:
        assert "hipDeviceSynchronize" not in body(path, sig), (path, sig)
    setup = body("capi_fastfir.hip", "int csdr_fastfir_batch_setup(")
    assert setup.count("hipDeviceSynchronize") == 1 and "switch to one filter per channel" in setup
    # the same-mode half of SetDemod: everything behind the `if (c.mode != mode)` block of apply_set_demod
    asd = body("chain_core.hpp", "int apply_set_demod(")
    tail = asd[asd.index("c.cw_off = info.Offset;"):]
    assert "pull(" not in tail and "push(" not in tail and "hipDeviceSynchronize" not in tail


def test_bench_fm_start_up_rule_is_the_derived_one():
    """bench.py's spot check of a timed FM buffer applies the per-burst bounds of tests/startup_bounds.py (the oracle's own
    spread x 2, counted from the burst in which the loop pulls in), not a fixed 1e-3 for the fourth burst."""
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    bench = importlib.import_module("bench")
    import startup_bounds as SB
    hop, fs = 1024, bench.FULL_SCALE
    want = np.zeros(12 * hop)
    def errs(per_burst):
        got = want.copy()
        for b, e in enumerate(per_burst):
            got[b * hop + 5] = e * fs
        return got
    bounds = [SB.FACTOR * s for s in SB.FM_SPREAD[1:]]
    # pull-in in burst 0 (arbitrary there), then just inside every bound
    ok = bench.chain_burst_check(errs([1.5] + [0.99 * b for b in bounds] + [2.9e-5] * 6), want, "FM")
    assert ok["ok"] and ok["tolerance_steady"] == 3e-5
    # the same stream with the pull-in one burst later (a 10 MSPS chain: its first burst is silent on both sides)
    assert bench.chain_burst_check(errs([0.0, 1.5] + [0.99 * b for b in bounds] + [2.9e-5] * 5), want, "FM")["ok"]
    # one burst over its bound fails, whichever it is
    for k in range(len(bounds)):
        e = [1.5] + [0.99 * b for b in bounds] + [2.9e-5] * 6
        e[1 + k] = 1.01 * bounds[k]
        assert not bench.chain_burst_check(errs(e), want, "FM")["ok"], k
    assert not bench.chain_burst_check(errs([1.5] + [0.99 * b for b in bounds] + [3.1e-5] * 6), want, "FM")["ok"]
