"""GPU parity of the 16384-point real-gain overlap-save kernel on its radix-4 tail groups (fastfir2_kernels.hip: K1_RADIX4,
fft_core.hpp: dit_tail_r4 / dit_tail_middle_r4) against the fp64 oracle.

The groups change the rounding order of the last two stages of all six register networks of fastfir_os2_kernel<14> and
nothing else: same twiddle sets, same upload order, same kernel for every other size and for complex H.  What can go wrong is
a constant of one group (a ratio m_gamma / m_beta, a rotation by j): that moves four of a network's rows by O(1) of their
value, far outside the bound.  Three filters in turn over the channels (an even pass band alone would hide a sign), 3 and 8
channels (the two channel -> workgroup maps), 1 / 2 / 3 / 8 blocks per call (single block, pair, odd tail, runs), two calls
per case so that the second runs on the overlap the first left, host and device design, every launch's kernel asserted; and
full-scale impulses at an even and an odd sample against the taps.  Bound: the kernels' |err| <= 2e-5 * max|x| per sample."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 2e-5
N, HOP = 16384, 8192
PIPELINED_GAIN = 2                                      # FastFirKernel, fastfir_kernels.h
FILTERS = [(-250, 250, 700, 48000.0), (300, 2700, -800, 48000.0), (-5000, 5000, 0, 48000.0)]
worst = {"err": 0.0}


def lib():
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__fastfir_set_variant.restype = C.c_int
    L.csdr__fastfir_set_variant.argtypes = [C.c_void_p, C.c_int]
    L.csdr__fastfir_last_kernel.restype = C.c_int
    L.csdr__fastfir_last_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.csdr__host_fastfir2_radix4.restype = C.c_int
    return L


def last_kernel(b):
    k, tw = C.c_int(-2), C.c_int(-2)
    assert lib().csdr__fastfir_last_kernel(b.h, C.byref(k), C.byref(tw)) == 0
    return k.value


def make(Cn, on_device):
    import cutesdr_amd as ca
    b = ca.FastFirBatch(Cn, N)
    flt = [FILTERS[c % 3] for c in range(Cn)]
    if on_device:
        b.setup(-5000, 5000, 0, 62500.0, channel=0)          # (per-channel filters first: the one call that reallocates)
        st = b.setup_many(list(range(Cn)), [f[0] for f in flt], [f[1] for f in flt], [f[2] for f in flt], [f[3] for f in flt])
        assert (st == 1).all()
    else:
        for c, f in enumerate(flt):
            assert b.setup(*f, channel=c) == 1
    assert lib().csdr__fastfir_set_variant(b.h, 2) == 0
    return b


_refs = {}


def reference(oracle, Cn, nb):
    """two consecutive calls of nb blocks through the fp64 oracle, once per shape: (x [call, channel, sample], y [channel, sample])"""
    if (Cn, nb) not in _refs:
        rng = np.random.default_rng(1000 * Cn + nb)
        x = (3000.0 * (rng.standard_normal((2, Cn, nb * HOP)) + 1j * rng.standard_normal((2, Cn, nb * HOP)))).astype(np.complex64)
        ref = []
        for c in range(Cn):
            ff = oracle.CFastFIR(N)
            assert ff.SetupParameters(*FILTERS[c % 3]) == 1
            ref.append(np.concatenate([ff.ProcessData(x[0, c].astype(np.complex128)), ff.ProcessData(x[1, c].astype(np.complex128))]))
        ref = np.stack(ref)
        x.setflags(write=False)
        ref.setflags(write=False)
        _refs[(Cn, nb)] = (x, ref)
    return _refs[(Cn, nb)]


def test_the_library_runs_the_radix4_form():
    assert lib().csdr__host_fastfir2_radix4() == 1


@pytest.mark.parametrize("on_device", [False, True], ids=["host_design", "device_design"])
@pytest.mark.parametrize("nb", [1, 2, 3, 8])
@pytest.mark.parametrize("Cn", [3, 8])
def test_radix4_kernel_matches_the_oracle(oracle, Cn, nb, on_device):
    x, ref = reference(oracle, Cn, nb)
    b = make(Cn, on_device)
    assert last_kernel(b) == -1
    y = []
    for call in (0, 1):
        y.append(b.process(x[call]))
        assert last_kernel(b) == PIPELINED_GAIN, (Cn, nb, call, last_kernel(b))
    b.close()
    err = np.abs(np.concatenate(y, axis=1) - ref).max(axis=1) / np.abs(x).max()
    worst["err"] = max(worst["err"], float(err.max()))
    print("C=%d blocks=%d %s: max err / max|x| per channel %s; largest so far %.3g"
          % (Cn, nb, "device_design" if on_device else "host_design", err, worst["err"]))
    assert (err <= TOL).all(), (Cn, nb, err)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_design", "device_design"])
@pytest.mark.parametrize("at", [1000, 4097], ids=["even_index", "odd_index"])
def test_impulse_gives_the_taps(at, on_device):
    """a full-scale impulse at sample `at`: the output is the 8193 taps from sample `at` on and zero elsewhere"""
    Cn, nb, A = 3, 3, 32767.0
    x = np.zeros((Cn, nb * HOP), dtype=np.complex64)
    x[:, at] = A
    b = make(Cn, on_device)
    y = b.process(x)
    assert last_kernel(b) == PIPELINED_GAIN
    for c in range(Cn):
        taps = np.fft.fft(b.response(c))[:HOP + 1]          # h[i] = sum_k H[k] e^{-j 2 pi i k / N} (H carries the 1/N)
        want = np.zeros(nb * HOP, dtype=np.complex128)
        want[at:at + HOP + 1] = A * taps
        err = np.abs(y[c] - want).max()
        print("impulse at %d, %s, channel %d: max err / A = %.3g (largest tap %.3g)"
              % (at, "device_design" if on_device else "host_design", c, err / A, np.abs(taps).max()))
        assert err <= TOL * A, (c, err / A)
    b.close()
