"""GPU parity of the pipelined overlap-save kernels against the fp64 oracle where the upload order of H / the gains goes
through fastfir2_slot_bin (fastfir2_kernels.hip, the shared twiddles).

The two 16384-point kernels (real gains, complex H) run on SHARED twiddles: rows k1 and 32 - k1 of the radix-32 passes on
one table entry, rows k0 and 16 - k0 of the outer pass on one twiddle power, and the rows / sub-transforms that took the
conjugate hold their bins rotated by one -- which only the upload order accounts for.  A wrong or missing rotation moves
fifteen of every thirty-two bins by N / 32: tests/test_fastfir_twshare.py shows, for the narrow filter used here, that such
an upload is off by more than 100 x this file's bound.  At N = 2048, 4096 and 8192 the kernels keep a twiddle per row
(DESIGN.md, K1): there the cases check only that the composed order is the base order, i.e. that those sizes still compute
what they did.

The three filters differ per channel (an even pass band alone would hide a sign), the hop counts cover block pairs and the
odd tail, the second call of every case runs on the overlap the first one left, responses are designed on the host and on
the device.  Tolerance: the kernels' |err| <= 2e-5 * max|x| per sample."""
import ctypes as C
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 2e-5
GENERIC, PIPELINED_H, PIPELINED_GAIN = 0, 1, 2          # FastFirKernel, fastfir_kernels.h
FILTERS = [(-250, 250, 700, 48000.0), (300, 2700, -800, 48000.0), (-5000, 5000, 0, 48000.0)]
SIZES = [2048, 4096, 8192, 16384]
worst = {}                                              # size -> largest err / max|x| seen so far


def lib():
    import cutesdr_amd as ca
    L = ca.lib()
    L.csdr__fastfir_set_variant.restype = C.c_int
    L.csdr__fastfir_set_variant.argtypes = [C.c_void_p, C.c_int]
    L.csdr__fastfir_set_own_design.restype = C.c_int
    L.csdr__fastfir_set_own_design.argtypes = [C.c_void_p, C.c_int]
    L.csdr__fastfir_last_kernel.restype = C.c_int
    L.csdr__fastfir_last_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.csdr__fastfir_batch_copy_row.restype = C.c_int
    L.csdr__fastfir_batch_copy_row.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.csdr__host_fastfir2_twshare.restype = C.c_int
    return L


def last_kernel(b):
    k, tw = C.c_int(-2), C.c_int(-2)
    assert lib().csdr__fastfir_last_kernel(b.h, C.byref(k), C.byref(tw)) == 0
    return k.value


def make(n, filters, on_device, own_design=True):
    import cutesdr_amd as ca
    b = ca.FastFirBatch(len(filters), n)
    if on_device:
        b.setup(-5000, 5000, 0, 62500.0, channel=0)          # (per-channel filters first: the one call that reallocates)
        st = b.setup_many(list(range(len(filters))), [f[0] for f in filters], [f[1] for f in filters],
                          [f[2] for f in filters], [f[3] for f in filters])
        assert (st == 1).all()
    else:
        for c, f in enumerate(filters):
            assert b.setup(*f, channel=c) == 1
    assert lib().csdr__fastfir_set_variant(b.h, 2) == 0
    if not own_design:
        assert lib().csdr__fastfir_set_own_design(b.h, 0) == 0
    return b


_refs = {}


def reference(oracle, n, nb):
    """two consecutive calls of nb hops through the fp64 oracle, once per shape: (x [call, channel, sample], y [channel, sample])"""
    if (n, nb) not in _refs:
        hop = n // 2
        rng = np.random.default_rng(n + nb)
        x = (3000.0 * (rng.standard_normal((2, 3, nb * hop)) + 1j * rng.standard_normal((2, 3, nb * hop)))).astype(np.complex64)
        ref = []
        for c in range(3):
            ff = oracle.CFastFIR(n)
            assert ff.SetupParameters(*FILTERS[c]) == 1
            ref.append(np.concatenate([ff.ProcessData(x[0, c].astype(np.complex128)), ff.ProcessData(x[1, c].astype(np.complex128))]))
        ref = np.stack(ref)
        x.setflags(write=False)
        ref.setflags(write=False)
        _refs[(n, nb)] = (x, ref)
    return _refs[(n, nb)]


def run_case(oracle, n, nb, on_device, own_design):
    x, ref = reference(oracle, n, nb)
    kernel = PIPELINED_GAIN if (n == 16384 and own_design) else PIPELINED_H
    b = make(n, FILTERS, on_device, own_design)
    assert last_kernel(b) == -1
    y = []
    for call in (0, 1):
        y.append(b.process(x[call]))
        assert last_kernel(b) == kernel, (n, nb, call, last_kernel(b))
    b.close()
    err = np.abs(np.concatenate(y, axis=1) - ref).max(axis=1) / np.abs(x).max()
    worst[n] = max(worst.get(n, 0.0), float(err.max()))
    print("N=%d hops=%d %s %s: max err / max|x| per channel %s; largest at this size so far %.3g"
          % (n, nb, "device_design" if on_device else "host_design", "own_design" if own_design else "complex_h", err, worst[n]))
    assert (err <= TOL).all(), (n, nb, err)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_design", "device_design"])
@pytest.mark.parametrize("nb", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_shared_twiddle_kernels_match_the_oracle(oracle, n, nb, on_device):
    if n == 16384:
        assert lib().csdr__host_fastfir2_twshare() >= 1      # the 16384-point kernels of the product's build share the twiddles
    run_case(oracle, n, nb, on_device, True)


@pytest.mark.parametrize("on_device", [False, True], ids=["host_design", "device_design"])
@pytest.mark.parametrize("nb", [1, 2, 3])
def test_16384_points_on_complex_h_match_the_oracle(oracle, nb, on_device):
    """own_design cleared: the same launches go to fastfir_os2h_kernel, whose H is uploaded through the rotated order too"""
    run_case(oracle, 16384, nb, on_device, False)


def test_copy_row_at_16384_points_takes_the_rotated_tables(oracle):
    """source row 1 continues as destination row 0 behind the first call: from there the destination row's words are the
    source row's own, and both are the oracle's stream"""
    n, nb = 16384, 2
    x, ref = reference(oracle, n, nb)
    cut = nb * (n // 2)
    src = make(n, FILTERS, False)
    dst = make(n, [FILTERS[2], FILTERS[0]], False)
    ys0 = src.process(x[0])
    dst.process(x[0][[2, 0]])
    assert lib().csdr__fastfir_batch_copy_row(dst.h, 0, src.h, 1) == 0
    ys1 = src.process(x[1])
    yd1 = dst.process(x[1][[1, 0]])
    assert last_kernel(src) == PIPELINED_GAIN and last_kernel(dst) == PIPELINED_GAIN
    src.close(); dst.close()
    err = np.abs(np.concatenate([ys0, ys1], axis=1) - ref).max() / np.abs(x).max()
    errd = np.abs(yd1[0] - ref[1, cut:]).max() / np.abs(x).max()
    print("copy_row N=16384: source max err / max|x| = %.3g, destination row behind the copy %.3g" % (err, errd))
    assert err <= TOL and errd <= TOL
    assert np.array_equal(yd1[0].view(np.uint32), ys1[1].view(np.uint32))
