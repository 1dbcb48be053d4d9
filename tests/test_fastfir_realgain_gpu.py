"""GPU parity of the 16384-point overlap-save kernel on REAL GAINS (the response of the library's own design is
H[k] = P[k] j^k: a real scale and a shift of the block by N/4 samples, fastfir2_kernels.hip) against the fp64 oracle and
against the generic kernel on complex H.  Tolerance: the kernel's |err| <= 2e-5 * max|x| per sample.  An asymmetric pass
band and a CW offset are where a wrong sign of the shift or a wrong row window is a gross error; the impulses pin the shift
sample by sample.

Which kernel a launch took is not left to the build's defaults: csdr__fastfir_last_kernel reports what
fastfir2_launch chose, and every case asserts it -- a real-gain case that had quietly run on complex H would otherwise
pass and prove nothing.  csdr__fastfir_set_own_design(0) is what a setter of raw responses will do: the same launches then
go to fastfir_os2h_kernel, the pipelined kernel on complex H, under the same cases (the third column, "complex_h").
The file also runs against other builds of K1 (tests/test_fastfir_twreg_gpu.py): CSDR_EXPECT_K1_TWREG is then the
K1_TWREG the library under CSDR_LIB_PATH must report."""
import ctypes as C
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 2e-5
N, HOP = 16384, 8192
GENERIC, PIPELINED_H, PIPELINED_GAIN = 0, 1, 2          # FastFirKernel, fastfir_kernels.h
# column -> (variant, own_design, the kernel its launches must take)
COLUMNS = {"generic": (0, True, GENERIC), "real_gain": (2, True, PIPELINED_GAIN), "complex_h": (2, False, PIPELINED_H)}
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
    L.csdr__fastfir_set_own_design.restype = C.c_int
    L.csdr__fastfir_set_own_design.argtypes = [C.c_void_p, C.c_int]
    L.csdr__fastfir_last_kernel.restype = C.c_int
    L.csdr__fastfir_last_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.csdr__fastfir_batch_copy_row.restype = C.c_int
    L.csdr__fastfir_batch_copy_row.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    return L


def last_kernel(b):
    """(kernel of b's most recent process call, K1_TWREG of the library)"""
    k, tw = C.c_int(-2), C.c_int(-2)
    assert lib().csdr__fastfir_last_kernel(b.h, C.byref(k), C.byref(tw)) == 0
    return k.value, tw.value


@pytest.fixture(scope="module", autouse=True)
def library_is_the_build_asked_for():
    """under tests/test_fastfir_twreg_gpu.py: the library loaded really is the one compiled with that K1_TWREG"""
    want = os.environ.get("CSDR_EXPECT_K1_TWREG")
    if want is not None:
        import cutesdr_amd as ca
        b = ca.FastFirBatch(1, 2048)
        kernel, twreg = last_kernel(b)
        b.close()
        assert kernel == -1 and twreg == int(want), (kernel, twreg, want, os.environ.get("CSDR_LIB_PATH"))


def make(Cn, variant, on_device, own_design=True, n=N):
    import cutesdr_amd as ca
    b = ca.FastFirBatch(Cn, n)
    if on_device:
        b.setup(-5000, 5000, 0, 62500.0, channel=0)          # (per-channel filters first: the one call that reallocates)
        flt = [filter_of(c) for c in range(Cn)]
        st = b.setup_many(list(range(Cn)), [f[0] for f in flt], [f[1] for f in flt], [f[2] for f in flt], [f[3] for f in flt])
        assert (st == 1).all()
    else:
        for c in range(Cn):
            assert b.setup(*filter_of(c), channel=c) == 1
    assert lib().csdr__fastfir_set_variant(b.h, variant) == 0
    if not own_design:
        assert lib().csdr__fastfir_set_own_design(b.h, 0) == 0
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
    for col, (v, own, kernel) in COLUMNS.items():
        b = make(Cn, v, on_device, own)
        assert last_kernel(b)[0] == -1
        y = []
        for call in (0, 1):
            y.append(b.process(x[call]))
            assert last_kernel(b)[0] == kernel, (col, call, last_kernel(b))
        outs[col] = np.concatenate(y, axis=1)
        b.close()
    tol = TOL * np.abs(x).max()
    for col in ("real_gain", "complex_h", "generic"):
        err = np.abs(outs[col] - ref).max(axis=1)
        print("C=%d blocks=%d %s: max err / max|x| per channel" % (Cn, nb, col), err / np.abs(x).max())
        assert (err <= tol).all(), (col, err / np.abs(x).max())
    assert np.abs(outs["real_gain"] - outs["generic"]).max() <= tol
    assert np.abs(outs["complex_h"] - outs["generic"]).max() <= tol


@pytest.mark.parametrize("at", [1000, 4097], ids=["even_index", "odd_index"])
def test_impulse_gives_the_taps_at_the_right_delay(at):
    """a full-scale impulse at sample `at`: the output is the 8193 taps from sample `at` on and zero elsewhere -- on real
    gains and, with own_design cleared, on complex H"""
    Cn, nb, A = 3, 3, 32767.0
    x = np.zeros((Cn, nb * HOP), dtype=np.complex64)
    x[:, at] = A
    for col in ("real_gain", "complex_h"):
        v, own, kernel = COLUMNS[col]
        b = make(Cn, v, False, own)
        y = b.process(x)
        assert last_kernel(b)[0] == kernel, (col, last_kernel(b))
        for c in range(Cn):
            taps = np.fft.fft(b.response(c))[:HOP + 1]          # h[i] = sum_k H[k] e^{-j 2 pi i k / N} (H carries the 1/N)
            want = np.zeros(nb * HOP, dtype=np.complex128)
            want[at:at + HOP + 1] = A * taps
            err = np.abs(y[c] - want).max()
            print("impulse at %d, %s, channel %d: max err / A = %.3g (largest tap %.3g)" % (at, col, c, err / A, np.abs(taps).max()))
            assert err <= TOL * A, (col, c, err / A)
        b.close()


def test_smaller_sizes_report_the_pipelined_kernel_on_complex_h():
    """below 16384 points there are no gains: variant 2 is the pipelined kernel on complex H whatever own_design says"""
    x = np.zeros((2, 2048), dtype=np.complex64)
    for v, kernel in ((2, PIPELINED_H), (0, GENERIC)):
        b = make(2, v, False, n=2048)
        b.process(x)
        assert last_kernel(b)[0] == kernel
        b.close()


# ---- csdr__fastfir_batch_copy_row at 16384 points: what csdr_demod_batch_set_demod calls when a receiver moves to another
# plan group.  The row takes the overlap, the complex response in both kernels' orders and the gains with it.
CALLS = (3, 3, 2)                      # hops per call: the copy is behind the first


def second_filter_of(c):
    """the filter a source row changes to behind its first call: another kind than its first"""
    return filter_of((c + 1) % 3 + 3)


def dst_filter_of(c):
    return filter_of((c + 2) % 3 + 6)


_copy_refs = {}


def copy_reference(oracle):
    """source: 3 rows, filter_of, then second_filter_of from the second call on; destination: 2 rows on other noise"""
    if not _copy_refs:
        rng = np.random.default_rng(77)
        T = sum(CALLS) * HOP
        xs = (3000.0 * (rng.standard_normal((3, T)) + 1j * rng.standard_normal((3, T)))).astype(np.complex64)
        xd = (3000.0 * (rng.standard_normal((2, T)) + 1j * rng.standard_normal((2, T)))).astype(np.complex64)
        cut = CALLS[0] * HOP

        def run(x, f0, f1):
            ff = oracle.CFastFIR(N)
            assert ff.SetupParameters(*f0) == 1
            y = [ff.ProcessData(x[:cut].astype(np.complex128))]
            if f1 is not None:
                assert ff.SetupParameters(*f1) == 1
            y.append(ff.ProcessData(x[cut:].astype(np.complex128)))
            return np.concatenate(y)
        rs = np.stack([run(xs[c], filter_of(c), second_filter_of(c)) for c in range(3)])
        rd = np.stack([run(xd[c], dst_filter_of(c), None) for c in range(2)])
        for a in (xs, xd, rs, rd):
            a.setflags(write=False)
        _copy_refs["r"] = (xs, xd, rs, rd)
    return _copy_refs["r"]


@pytest.mark.parametrize("src_own", [True, False], ids=["own_design", "own_design_cleared"])
@pytest.mark.parametrize("on_device", [False, True], ids=["host_design", "device_design"])
def test_copy_row_takes_overlap_response_and_gains(oracle, on_device, src_own):
    """Source row 1 continues as destination row 0 behind the first call.  The source's filters change in the same gap --
    designed on the host (the patches still queued) or through setup_many (the jobs still queued: the response copy_row
    has to fetch exists nowhere yet) -- so the destination gets a response it has never had, and with stale gains, a stale
    complex H or a missing overlap its very first samples are wrong.  From there the destination row is the oracle's
    stream of source row 1, word for word what the source row itself gives; every other row of both objects is untouched;
    both objects stay on the real-gain kernel -- unless the source's own_design was cleared: then the destination too
    runs on complex H."""
    xs, xd, rs, rd = copy_reference(oracle)
    L = lib()
    src = make(3, 2, False, src_own)
    dst = make(2, 2, False)
    for c in range(2):
        assert dst.setup(*dst_filter_of(c), channel=c) == 1
    src_kernel = PIPELINED_GAIN if src_own else PIPELINED_H
    bounds = np.cumsum((0,) + CALLS) * HOP
    ys, yd = [], []
    for k in range(len(CALLS)):
        a, e = bounds[k], bounds[k + 1]
        xin = xd[:, a:e].copy()
        if k >= 1:
            xin[0] = xs[1, a:e]                    # the moved stream goes on in destination row 0
        ys.append(src.process(xs[:, a:e]))
        yd.append(dst.process(xin))
        assert last_kernel(src)[0] == src_kernel, (k, last_kernel(src))
        assert last_kernel(dst)[0] == (PIPELINED_GAIN if (k == 0 or src_own) else PIPELINED_H), (k, last_kernel(dst))
        if k == 0:
            flt = [second_filter_of(c) for c in range(3)]
            if on_device:
                st = src.setup_many([0, 1, 2], [f[0] for f in flt], [f[1] for f in flt], [f[2] for f in flt], [f[3] for f in flt])
                assert (st == 1).all()
            else:
                for c in range(3):
                    assert src.setup(*flt[c], channel=c) == 1
            assert L.csdr__fastfir_batch_copy_row(dst.h, 0, src.h, 1) == 0
    ys, yd = np.concatenate(ys, axis=1), np.concatenate(yd, axis=1)
    cut = bounds[1]
    tol = TOL * max(np.abs(xs).max(), np.abs(xd).max())
    err = {"source rows": np.abs(ys - rs).max(axis=1), "destination row 1": np.abs(yd[1] - rd[1]).max(),
           "destination row 0 before the copy": np.abs(yd[0, :cut] - rd[0, :cut]).max(),
           "destination row 0 behind the copy": np.abs(yd[0, cut:] - rs[1, cut:]).max(),
           "its first hop": np.abs(yd[0, cut:cut + HOP] - rs[1, cut:cut + HOP]).max()}
    for what, e in err.items():
        print("copy_row %s: max err / max|x|" % what, e / (tol / TOL))
        assert np.all(e <= tol), (what, e / (tol / TOL))
    assert np.array_equal(yd[0, cut:].view(np.uint32), ys[1, cut:].view(np.uint32))
    src.close(); dst.close()
