"""A bin-resolving measure of the display spectrum (K3: CFft::PutInDisplayFFT -- window, I/Q swap, transform, power,
running mean, log10) -- TEST INFRASTRUCTURE, imported by name like k1_bins.py, whose probe and margins it reuses.

The probe is k1_bins.probe: a flat spectrum, 3000 rms, complex64, crest factor at most 3.3 (it never reaches the overload
limit), a distinct seed per frame and per row (seed_of).  The reference is the fp64 oracle's CFft fed frame by frame on
the widened complex64 words.

The figure compares bels as amplitudes, decoded in fp64:
    A[j] = sqrt(max(10**(b[j] - K_B) - K_C, 0)),    K_B, K_C those of fft.cpp:186-188 for the size and the compensation,
    E = max_j |A_got[j] - A_ref[j]| / sqrt(mean_j P_ref[j]),      P_ref = A_ref**2, the oracle's mean power.
A windowed probe has deep Rayleigh nulls, where a bel -- or a relative error -- is unbounded; in amplitudes every bin
counts against the same scale, the rms bin amplitude, and none is left out.  decode() asserts that the clamp at 0 touches
no bin of a reference.

The yardstick E_y is the same figure of Yard32, an fp32 restatement of the whole pipeline on the CPU and never the code
under test: the window table rounded to fp32 from the reference's fp64 formula, the I/Q swap, scipy.fft on complex64
with the oracle's sign (the dtype asserted), the power in fp32, the reference's recursion (sum - mean + p, sum / count)
in fp32, an fp32 log10, + K_B in double, rounded to fp32.  It contains the bel's own quantisation, which on the CPU is
of the order of the transform's error, so one number bounds both.

The rule is E <= m E_y with m = margin(n) = fft_plain_ref.margin(n), the project's 4 and 6.43 at 16384 points (the outer
twiddles from the fp32 product tree).  Nothing here is imported by the product."""
import numpy as np
import scipy.fft

import fft_plain_ref
import k1_bins

SIZES = fft_plain_ref.SIZES
FS = 2.0e6
K_AMPMAX, K_MINDB, OVER_LIMIT = 32767.0, -220.0, 32000.0          # fft.cpp:19-23 (tests/golden/reference_constants.json)


def margin(n):
    """the plain transforms' margin; no size needed one of its own (measured on the MI355X: at most 2.77 E_y, at 4096
    points; per size in DESIGN.md, K3 parity)"""
    return fft_plain_ref.margin(n)


def consts(n, db_comp=0.0):
    """(K_B, K_C) of fft.cpp:186-188, K_B in bels"""
    kb = db_comp - 20.0 * np.log10(n * K_AMPMAX / 2.0)
    kc = 10.0 ** ((K_MINDB - kb) / 10.0)
    return kb / 10.0, kc


def window64(n):
    """the reference's window (fft.cpp:196-198): Hann times 2"""
    return 2.0 * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / (n - 1)))


def seed_of(n, row, frame, case=0):
    """a seed of its own for every (size, test case, row, frame)"""
    return ((int(np.log2(n)) * 64 + case) * 64 + row) * 256 + frame


def frames(n, rows, nframes, case=0, first=0):
    """[rows, nframes, n] complex64: frame `first + k` of every row, each from its own seed"""
    return np.stack([np.stack([fft_plain_ref.probe(n, seed_of(n, r, first + k, case)) for k in range(nframes)])
                     for r in range(rows)])


def decode(bels, n, db_comp=0.0, reference=False):
    """bels -> amplitudes, in fp64.  reference: the clamp at 0 must touch no bin"""
    kb, kc = consts(n, db_comp)
    p = 10.0 ** (np.asarray(bels, dtype=np.float64) - kb) - kc
    if reference:
        assert (p > 0.0).all(), "the clamp leaves %d bins of the reference out" % int((p <= 0.0).sum())
    return np.sqrt(np.maximum(p, 0.0))


def figure(got, ref, n, db_comp=0.0):
    """E of the bels `got` against the oracle's bels `ref`"""
    got = np.asarray(got)
    assert got.shape == (n,) and np.isfinite(got).all()
    a_ref = decode(ref, n, db_comp, reference=True)
    return float(np.abs(decode(got, n, db_comp) - a_ref).max() / np.sqrt(np.mean(a_ref ** 2)))


class Yard32:
    """CFft's display side in fp32 on the CPU: SetFFTParams(n, ., db_comp, .), SetFFTAve, PutInDisplayFFT, m_pFFTAveBuf.
    The hooks plant faults on this side only: win_fault(w32) -> w32 once, power_fault(p, frame index) -> p per frame."""

    def __init__(self, n, ave, db_comp=0.0, win_fault=None, power_fault=None):
        self.n, self.db_comp = n, db_comp
        self.kb, kc = consts(n, db_comp)
        self.kc = np.float32(kc)
        self.win = window64(n).astype(np.float32)
        if win_fault is not None:
            self.win = np.asarray(win_fault(self.win.copy()), dtype=np.float32)
        self.power_fault = power_fault
        self.ave_size = 1
        self.put_count = 0
        self.SetFFTAve(ave)

    def SetFFTAve(self, ave):                            # fft.cpp:103-113, ends in ResetFFT (:248-259)
        self.ave_size = ave if ave > 0 else 1
        self.sum = np.zeros(self.n, dtype=np.float32)
        self.mean = np.zeros(self.n, dtype=np.float32)
        self.bels = np.zeros(self.n, dtype=np.float32)
        self.ave_count = self.total = 0

    def PutInDisplayFFT(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        assert x.shape == (self.n,)
        y = np.empty(self.n, dtype=np.complex64)
        y.real = self.win * x.imag                       # fft.cpp:280-281: I and Q swapped
        y.imag = self.win * x.real
        X = scipy.fft.ifft(y, norm="forward")            # the positive exponent, unnormalised: the oracle's sign
        assert X.dtype == np.complex64, X.dtype          # (numpy.fft upcasts on older numpy; scipy.fft does not)
        p = np.fft.fftshift(X.real * X.real + X.imag * X.imag)      # display order, fft.cpp:564-589
        assert p.dtype == np.float32
        if self.power_fault is not None:
            p = np.asarray(self.power_fault(p.copy(), self.put_count), dtype=np.float32)
        self.put_count += 1
        self.total += 1                                  # fft.cpp:515-517
        if self.ave_count < self.ave_size:
            self.ave_count += 1
        if self.total <= self.ave_size:                  # fft.cpp:570-574
            self.sum = self.sum + p
        else:
            self.sum = self.sum - self.mean + p
        self.mean = self.sum / np.float32(self.ave_count)
        lg = np.log10(self.mean + self.kc)
        assert self.sum.dtype == self.mean.dtype == lg.dtype == np.float32
        self.bels = (lg.astype(np.float64) + self.kb).astype(np.float32)
        return self.total

    def ave_buf(self):
        return self.bels.copy()


def oracle_fft(orc, n, ave, db_comp=0.0):
    r = orc.CFft()
    r.SetFFTParams(n, False, db_comp, FS)
    r.SetFFTAve(ave)
    return r


def feed(objs, x):
    """the frames x [nframes, n] into every object of objs, frame by frame (the complex64 words widened)"""
    for fr in x:
        wide = fr.astype(np.complex128)
        for o in objs:
            o.PutInDisplayFFT(wide)


def reference(orc, x, ave, db_comp=0.0):
    """(ref bels, E_y) of one row's frames x [nframes, n] put into a fresh object with average `ave`"""
    n = x.shape[1]
    r, y = oracle_fft(orc, n, ave, db_comp), Yard32(n, ave, db_comp)
    feed((r, y), x)
    ref = r.ave_buf()
    return ref, figure(y.ave_buf(), ref, n, db_comp)


def check(got, ref, e_y, n, what="", db_comp=0.0):
    """the rule for one row; prints and returns E / E_y"""
    e = figure(got, ref, n, db_comp)
    print("%s n=%d: E = %.3g = %.2f E_y (E_y = %.3g, m = %g)" % (what, n, e, e / e_y, e_y, margin(n)))
    assert e <= margin(n) * e_y, "%s n=%d: E = %.3g = %.2f E_y (E_y = %.3g, m = %g)" % (what, n, e, e / e_y, e_y, margin(n))
    return e / e_y
