"""CPU checks of the batch SetDemod: the three new entry points are declared, exported and bound; they answer CSDR_EHIP
without a GPU; and the host half of a device-side filter design (csdr__host_design_job: the reference's sanity check and
the two normalised doubles) accepts and rejects what the oracle's SetupParameters accepts and rejects and returns the
doubles bit-equal to a numpy restatement of host_math.hpp's statements."""
import ctypes as C
import numpy as np
import pytest

NEW = ["csdr_fastfir_batch_setup_many", "csdr_demod_batch_set_demod_many", "csdr_demod_shard_set_demod_many"]
TWO_PI = 2.0 * 3.14159265358979323846


@pytest.fixture(scope="module")
def L():
    from cutesdr_amd import _build, _capi
    _build.build()
    lib = _capi.lib()
    lib.csdr__host_design_job.restype = C.c_int
    lib.csdr__host_design_job.argtypes = [C.c_double] * 4 + [C.c_void_p, C.c_void_p]
    return lib


def test_new_symbols_are_declared_exported_and_bound(L):
    from cutesdr_amd import _capi
    import cutesdr_amd as ca
    P, I = C.c_void_p, C.c_int
    protos = _capi.prototypes()
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert name in protos, name
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.restype is I and list(fn.argtypes) == protos[name][1], name
    assert protos[NEW[0]] == (I, [P, I, P, P, P, P, P, P])
    assert protos[NEW[1]] == (I, [P, I, P, P, P, P])
    assert protos[NEW[2]] == (I, [P, I, P, P, P, P])
    assert callable(ca.FastFirBatch.setup_many) and callable(ca.DemodBatch.set_demod_many)
    assert callable(ca.ShardedDemodBatch.set_demod_many)


def test_entry_points_without_a_gpu(L):
    """no CPU fallback: without a device every new call is CSDR_EHIP and the objects cannot be made; with one, a null
    handle is CSDR_EINVAL"""
    from cutesdr_amd import _capi
    import cutesdr_amd as ca
    want = _capi.CSDR_EHIP if L.csdr_device_count() == 0 else _capi.CSDR_EINVAL
    one = (C.c_int * 1)(0)
    d = (C.c_double * 1)(1.0)
    info = ca.fm_defaults()
    assert L.csdr_fastfir_batch_setup_many(None, 1, one, d, d, d, d, one) == want
    assert L.csdr_demod_batch_set_demod_many(None, 1, one, one, C.byref(info), one) == want
    assert L.csdr_demod_shard_set_demod_many(None, 1, one, one, C.byref(info), one) == want
    if L.csdr_device_count() == 0:
        assert b"no HIP device" in L.csdr_last_error()
        for make in (lambda: ca.FastFirBatch(2, 2048), lambda: ca.DemodBatch(2), lambda: ca.ShardedDemodBatch([0], 2)):
            with pytest.raises(_capi.CsdrError):
                make()


def _numpy_job(flo, fhi, off, fs):
    flo, fhi, off, fs = (np.float64(v) for v in (flo, fhi, off, fs))
    flo = flo + off
    fhi = fhi + off
    nfl, nfh = flo / fs, fhi / fs
    return (nfh - nfl) / np.float64(2.0), np.float64(TWO_PI) * (nfh + nfl) / np.float64(2.0)


def test_host_design_job_accepts_rejects_and_normalises_like_the_reference(L, oracle):
    rng = np.random.default_rng(20260)
    cases = []
    for _ in range(300):
        fs = float(rng.choice([15625.0, 31250.0, 62500.0, 48000.0, 7812.5]))
        lo, hi = sorted(rng.uniform(-0.6 * fs, 0.6 * fs, 2))
        if rng.random() < 0.1:
            lo, hi = hi, lo
        off = float(rng.choice([0.0, 700.0, -700.0, rng.uniform(-2000, 2000)]))
        cases.append((float(np.round(lo)), float(np.round(hi)), off, fs))
    fs = 62500.0
    h, inside, outside = fs / 2.0, np.nextafter(fs / 2.0, 0.0), np.nextafter(fs / 2.0, 1e9)
    cases += [(-h, 100.0, 0.0, fs), (-inside, 100.0, 0.0, fs), (-outside, 100.0, 0.0, fs), (100.0, h, 0.0, fs),
              (100.0, inside, 0.0, fs), (100.0, outside, 0.0, fs), (500.0, 500.0, 0.0, fs), (500.0, np.nextafter(500.0, 1e9), 0.0, fs),
              (-250.0, 250.0, 700.0, fs), (-250.0, 250.0, -700.0, fs), (h - 700.0, h, -700.0, fs), (30000.0, 31000.0, 700.0, fs),
              (-31000.0, -30000.0, -700.0, fs), (-50.0, 50.0, 0.0, fs), (100.0, 2800.0, 0.0, fs), (-2800.0, -100.0, 0.0, fs)]
    accepted = rejected = 0
    for lo, hi, off, fs in cases:
        nfc, nfs = C.c_double(), C.c_double()
        got = L.csdr__host_design_job(lo, hi, off, fs, C.addressof(nfc), C.addressof(nfs))
        want = oracle.CFastFIR(2048).SetupParameters(lo, hi, off, fs)
        assert want in (1, -1), (lo, hi, off, fs, want)
        assert got == (0 if want == 1 else -1), (lo, hi, off, fs, got, want)
        if got == 0:
            accepted += 1
            a, b = _numpy_job(lo, hi, off, fs)
            assert nfc.value == float(a) and nfs.value == float(b), (lo, hi, off, fs)
        else:
            rejected += 1
    assert accepted > 50 and rejected > 20
