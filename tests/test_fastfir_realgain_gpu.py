"""GPU parity of the 16384-point overlap-save kernel on REAL GAINS (the response of the library's own design is
H[k] = P[k] j^k: a real scale and a shift of the block by N/4 samples, fastfir2_kernels.hip) against the fp64 oracle and
against the generic kernel on complex H.  Tolerance: the kernel's |err| <= 2e-5 * max|x| per sample.  An asymmetric pass
band and a CW offset are where a wrong sign of the shift or a wrong row window is a gross error; the impulses pin the shift
sample by sample."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 2e-5
N, HOP = 16384, 8192
BASE = [(100, 2800, 0, 48000.0), (-2800, -100, 0, 48000.0), (-250, 250, 700, 15625.0)]


def filter_of(c):
    """a distinct filter per channel: the three kinds in turn, edges moved a little from one channel to the next"""
    lo, hi, off, fs = BASE[c % 3]
    d = 7.0 * (c // 3)
    return (lo + d, hi + d, off, fs)


def lib():
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__fastfir_set_variant.restype = C.c_int
    L.csdr__fastfir_set_variant.argtypes = [C.c_void_p, C.c_int]
    return L


def make(Cn, variant, on_device):
    import cutesdr_amd as ca
    b = ca.FastFirBatch(Cn, N)
    if on_device:
        b.setup(-5000, 5000, 0, 62500.0, channel=0)          # (per-channel filters first: the one call that reallocates)
        flt = [filter_of(c) for c in range(Cn)]
        st = b.setup_many(list(range(Cn)), [f[0] for f in flt], [f[1] for f in flt], [f[2] for f in flt], [f[3] for f in flt])
        assert (st == 1).all()
    else:
        for c in range(Cn):
            assert b.setup(*filter_of(c), channel=c) == 1
    assert lib().csdr__fastfir_set_variant(b.h, variant) == 0
    return b


_refs = {}


def reference(oracle, Cn, nb):
    """two consecutive calls of nb blocks through the fp64 oracle, once per shape"""
    if (Cn, nb) not in _refs:
        rng = np.random.default_rng(100 * Cn + nb)
        x = (3000.0 * (rng.standard_normal((2, Cn, nb * HOP)) + 1j * rng.standard_normal((2, Cn, nb * HOP)))).astype(np.complex64)
        ref = []
        for c in range(Cn):
            ff = oracle.CFastFIR(N)
            assert ff.SetupParameters(*filter_of(c)) == 1
            ref.append(np.concatenate([ff.ProcessData(x[0, c].astype(np.complex128)), ff.ProcessData(x[1, c].astype(np.complex128))]))
        x.setflags(write=False)
        _refs[(Cn, nb)] = (x, np.stack(ref))
    return _refs[(Cn, nb)]


@pytest.mark.parametrize("on_device", [False, True], ids=["host_design", "device_design"])
@pytest.mark.parametrize("nb", [1, 2, 3, 8])
@pytest.mark.parametrize("Cn", [3, 8])
def test_real_gain_kernel_matches_oracle_and_generic_kernel(oracle, Cn, nb, on_device):
    x, ref = reference(oracle, Cn, nb)
    outs = {}
    for v in (0, 2):
        b = make(Cn, v, on_device)
        outs[v] = np.concatenate([b.process(x[0]), b.process(x[1])], axis=1)
        b.close()
    tol = TOL * np.abs(x).max()
    for v in (2, 0):
        err = np.abs(outs[v] - ref).max(axis=1)
        print("C=%d blocks=%d variant %d: max err / max|x| per channel" % (Cn, nb, v), err / np.abs(x).max())
        assert (err <= tol).all(), (v, err / np.abs(x).max())
    assert np.abs(outs[2] - outs[0]).max() <= tol


@pytest.mark.parametrize("at", [1000, 4097], ids=["even_index", "odd_index"])
def test_impulse_gives_the_taps_at_the_right_delay(at):
    """a full-scale impulse at sample `at`: the output is the 8193 taps from sample `at` on and zero elsewhere"""
    Cn, nb, A = 3, 3, 32767.0
    x = np.zeros((Cn, nb * HOP), dtype=np.complex64)
    x[:, at] = A
    b = make(Cn, 2, False)
    y = b.process(x)
    for c in range(Cn):
        taps = np.fft.fft(b.response(c))[:HOP + 1]          # h[i] = sum_k H[k] e^{-j 2 pi i k / N} (H carries the 1/N)
        want = np.zeros(nb * HOP, dtype=np.complex128)
        want[at:at + HOP + 1] = A * taps
        err = np.abs(y[c] - want).max()
        print("impulse at %d, channel %d: max err / A = %.3g (largest tap %.3g)" % (at, c, err / A, np.abs(taps).max()))
        assert err <= TOL * A, (c, err / A)
    b.close()
