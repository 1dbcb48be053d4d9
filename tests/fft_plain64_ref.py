"""The measure of the fp64 batch transforms (csdr_fft_batch_fwd_f64 / _rev_f64, K3q) -- TEST INFRASTRUCTURE, imported by
name like fft_plain_ref.py, whose probe it widens.

Probe: fft_plain_ref.probe(n, seed) (flat spectrum, 3000 rms) widened to complex128 and turned by one fresh fp64 random
phase, so that its words are not fp32-representable and every bin of its transform still has magnitude sqrt(n) rms.
Checker: scipy.fft on np.clongdouble input (x87 80-bit, eps 1.08e-19): three decimal digits below anything fp64 can show.
    E = max_k |got_k - ref_k| / (sqrt(n) rms(x)),   taken in long double.
Yardstick E_y: the same figure of scipy.fft's complex128 transform of the probe (on these probes, by seed and sign,
5e-16 ... 7e-16 at 512 points, 8e-16 ... 1.1e-15 at 4096, 1.2e-15 ... 1.5e-15 at 65536).  The rule is E <= 4 E_y at every size (k1_bins.MARGIN: another factorisation and rounding order); there
is no larger allowance anywhere, because every twiddle is tabulated.  E of the fp64 oracle is computed beside them.
Every reference is computed once per (size, seed, sign) and handed out read-only.  Nothing here is imported by the product."""
import functools

import numpy as np
import pytest
import scipy.fft

import fft_plain_ref as P32
import k1_bins

SIZES = P32.SIZES
SIGNS = P32.SIGNS
MARGIN = k1_bins.MARGIN
FS = P32.FS
FOUR_STEP = tuple(n for n in SIZES if n >= 8192)             # the sizes that go through the work buffer in two launches
LD = np.longdouble
CLD = np.clongdouble
TWO_PI_LD = LD("6.283185307179586476925286766559")


def require_long_double():
    """the checker needs a long double that resolves fp64 roundings, and a scipy.fft that transforms in it"""
    if not np.finfo(LD).eps < 1e-18:
        pytest.skip("np.longdouble is no wider than fp64 here (eps = %g): no checker for the fp64 transforms" % np.finfo(LD).eps)
    y = scipy.fft.fft(np.zeros(8, dtype=CLD))
    if y.dtype != CLD or np.finfo(y.real.dtype).eps >= 1e-18:
        pytest.skip("scipy.fft transforms long double input in %s" % y.dtype)


seed_of = P32.seed_of


@functools.lru_cache(maxsize=None)
def probe(n, seed):
    phi = np.random.default_rng(seed + 7919).uniform(0.0, 2.0 * np.pi)
    p = P32.probe(n, seed).astype(np.complex128) * np.exp(1j * phi)
    assert not (p.real.astype(np.float32).astype(np.float64) == p.real).all()
    p.setflags(write=False)
    return p


def checker_fft(x, sign):
    """the long double transform: FwdFFT has the positive exponent, neither normalises"""
    x = np.ascontiguousarray(x, dtype=CLD)
    y = scipy.fft.ifft(x, norm="forward") if sign > 0 else scipy.fft.fft(x)
    assert y.dtype == CLD, y.dtype
    return y


def yard_fft(x, sign):
    """the independent fp64 transform"""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    y = scipy.fft.ifft(x, norm="forward") if sign > 0 else scipy.fft.fft(x)
    assert y.dtype == np.complex128, y.dtype
    return y


def rel_err(got, ref, x):
    n = len(x)
    d = np.abs(np.asarray(got).astype(CLD) - np.asarray(ref).astype(CLD)).max()
    return float(d / (np.sqrt(LD(n)) * LD(k1_bins.rms(x))))


def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=None)
def reference(n, seed, sign):
    """(ref, E_y, E_oracle) of probe(n, seed): the long double transform, and the errors of the yardstick and of the
    fp64 oracle against it"""
    require_long_double()
    x = probe(n, seed)
    ref = checker_fft(x, sign)
    ref.setflags(write=False)
    return ref, rel_err(yard_fft(x, sign), ref, x), rel_err(_oracle().fft(np.array(x), sign), ref, x)


def check_frame(got, n, seed, sign, what="", ref=None):
    """the rule for one frame; returns (E / E_y, E_oracle / E_y).  ref: another reference than the long double checker
    (the yardstick is then measured against it too)"""
    x = probe(n, seed)
    if ref is None:
        ref, e_y, e_o = reference(n, seed, sign)
    else:
        e_y, e_o = rel_err(yard_fft(x, sign), ref, x), float("nan")
    assert np.asarray(got).dtype == np.complex128, np.asarray(got).dtype
    e = rel_err(got, ref, x)
    assert np.isfinite(e) and e <= MARGIN * e_y, \
        "%s n=%d sign=%+d seed=%d: E = %.3g = %.2f E_y (E_y = %.3g, m = %g)" % (what, n, sign, seed, e, e / e_y, e_y, MARGIN)
    return e / e_y, e_o / e_y


def impulse_ref(n, m, sign, amp=3000.0):
    """the transform of amp delta[i - m]: amp exp(sign j 2 pi m k / n) in long double, the angle reduced in integers"""
    k = (np.arange(n, dtype=np.int64) * m) % n
    a = TWO_PI_LD * k.astype(LD) / LD(n)
    return LD(amp) * (np.cos(a) + 1j * sign * np.sin(a)).astype(CLD)


def words(a):
    """the array's 64-bit words, for word-for-word comparisons"""
    return np.ascontiguousarray(a).view(np.uint64)


# ---- the host table builder's restatement (cutesdr_amd/csrc/fft_tw64_host.hpp)
def table_entries(period, count):
    """W_period^m, m < count, as the builder is meant to form it: the angle reduced in integers to the first octant, the
    C library's long double cos / sin of it (through np.longdouble) rounded once to fp64, the other octants by symmetry
    -> float64 [count, 2].  A restatement of the builder's steps, not an independent proof of correct rounding: it shows
    that the library's table is what those steps give.  That the values are the angles' is shown independently, by the
    fp64 library's cos / sin, the unit circle, the axes and the diagonals (test_fft_plain64_host.py) and by the impulse
    tests on the device."""
    m = np.arange(count, dtype=np.int64) % period
    octant = period // 8
    q, r = m // octant, m % octant
    j = np.where(q & 1, octant - r, r)
    a = j.astype(LD) * TWO_PI_LD / LD(period)
    c, s = np.cos(a).astype(np.float64), np.sin(a).astype(np.float64)
    re = np.choose(q, [c, s, -s, -c, -c, -s, s, c])
    im = np.choose(q, [s, c, c, s, -s, -c, -c, -s])
    return np.stack([re, im], axis=1) + 0.0


def table(n):
    """the table csdr_fft_batch_prepare_f64 builds for n points"""
    if n < 8192:
        return table_entries(n, n)
    return np.concatenate([table_entries(256, 256), table_entries(n, 256)])
