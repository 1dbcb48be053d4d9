"""The measure of the batch plain transforms (csdr_fft_batch_fwd / _rev) -- TEST INFRASTRUCTURE, imported by name like
k1_bins.py, whose probe and margins it reuses.

The probe has a flat spectrum (k1_bins.probe: random phases, 3000 rms, complex64), so every output bin of its transform has
magnitude sqrt(n) rms and ONE number is the per-bin relative error of a transform `got` of the probe x:
    E = max_k |got_k - ref_k| / (sqrt(n) rms(x)),      ref = oracle.fft(x, sign) on the widened complex64 words (fp64).
The yardstick E_y is the same figure of an independent fp32 transform, scipy.fft (pocketfft) on the complex64 array:
ifft(x, norm="forward") for FwdFFT (the positive exponent, unnormalised), fft(x) for RevFFT.  The rule is E <= m E_y with
m = k1_bins.MARGIN (4: another factorisation and rounding order), but 6.43 at 16384 points, where fft_fwd_passes derives
its outer twiddles by the fp32 product tree that k1_bins.MARGINS grants that allowance at R0 = 16.
Every reference is computed once per (size, seed, sign) and handed out read-only.  Nothing here is imported by the product."""
import functools

import numpy as np
import scipy.fft

import k1_bins

SIZES = (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
SIGNS = (+1, -1)
RMS = k1_bins.RMS
FS = 48000.0


def margin(n):
    return k1_bins.MARGINS[(16384, 0)] if n == 16384 else k1_bins.MARGIN


def seed_of(n, i):
    return 1000 * int(np.log2(n)) + i


@functools.lru_cache(maxsize=None)
def probe(n, seed):
    p = k1_bins.probe(n, seed)
    p.setflags(write=False)
    return p


def yard_fft(x, sign):
    """the independent fp32 transform"""
    x = np.ascontiguousarray(x, dtype=np.complex64)
    y = scipy.fft.ifft(x, norm="forward") if sign > 0 else scipy.fft.fft(x)
    assert y.dtype == np.complex64, y.dtype          # (numpy.fft upcasts on older numpy; scipy.fft does not)
    return y


def rel_err(got, ref, x):
    n = len(x)
    return float(np.abs(np.asarray(got, dtype=np.complex128) - ref).max() / (np.sqrt(n) * k1_bins.rms(x)))


def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=None)
def reference(n, seed, sign):
    """(ref, E_y) of probe(n, seed): the fp64 checker's transform and the yardstick's error against it"""
    x = probe(n, seed)
    ref = _oracle().fft(x.astype(np.complex128), sign)
    ref.setflags(write=False)
    return ref, rel_err(yard_fft(x, sign), ref, x)


def check_frame(got, n, seed, sign, what="", ref=None):
    """the rule for one frame; returns E / E_y.  ref: another fp64 reference than the oracle's (the yardstick is then
    measured against it too)"""
    x = probe(n, seed)
    if ref is None:
        ref, e_y = reference(n, seed, sign)
    else:
        e_y = rel_err(yard_fft(x, sign), ref, x)
    e = rel_err(got, ref, x)
    assert np.isfinite(e) and e <= margin(n) * e_y, \
        "%s n=%d sign=%+d seed=%d: E = %.3g = %.2f E_y (E_y = %.3g, m = %g)" % (what, n, sign, seed, e, e / e_y, e_y, margin(n))
    return e / e_y


def impulse_ref(n, m, sign, amp=3000.0):
    """the transform of amp delta[i - m]: amp exp(sign j 2 pi m k / n), the angle reduced in integers"""
    k = (np.arange(n, dtype=np.int64) * m) % n
    return amp * np.exp(sign * 2j * np.pi * k / n)


def words(a):
    """the array's 32-bit words, for word-for-word comparisons"""
    return np.ascontiguousarray(a).view(np.uint32)
