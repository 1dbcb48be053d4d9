"""A bin-resolving measure of the overlap-save filter (K1) -- TEST INFRASTRUCTURE, imported by name like dc_ref.py.

The probe is N-periodic with a flat spectrum: p = ifft(exp(j phi_k)), phi_k uniform, 3000 rms, rounded to complex64 and
tiled.  Overlap-save blocks advance by N/2, so every block of such a stream holds a rotation of the same period: every
bin of every block carries the same magnitude, and from sample N on (the filter has N/2 + 1 taps) the output is
N-periodic too.  An N-point fp64 FFT of N consecutive output samples therefore gives the multiplier the kernel really
applied to every single bin, with no leakage, where white noise dilutes one bin's error by 1/N.

Figures of an output `got` against the fp64 oracle's `ref` on window w (samples [wN, (w+1)N), w >= 1), with e = got - ref,
E = fft(e), X = fft(x[N:2N]) and g = max_k |fft(ref)_k / X_k| (the peak effective gain):
    B = max_k |E_k| / (|X_k| g)        the largest error of one bin's multiplier, relative to the peak gain
    T = max |e| / (g rms(x))           the largest error of one sample
The yardstick is the same two figures of a plain fp32 transform pair on the CPU, scipy.fft.ifft(scipy.fft.fft(p32) Heff32)
on one period, against the fp64 product on the same complex64 multipliers Heff32 = fft(ref)/X: an independent fp32
evaluation of the same operation, never the code under test.  The parity rule is B <= m B_y and T <= m T_y with
m = margin(n, kernel): 4, but for the one kernel listed in MARGINS.
Nothing here is imported by the product."""
import numpy as np
import scipy.fft

RMS = 3000.0
PERIODS = 4                        # a stream: 4 periods = 8 hops
WINDOWS = (1, 2, 3)                # the steady windows of such a stream
MARGIN = 4.0                       # another factorisation and rounding order than the yardstick's: a factor of 4, no more
# One kernel has a margin of its own.  The generic kernel (fastfir_kernels.hip) keeps one outer-pass twiddle W_N^n2 per column
# and derives W_N^(k0 n2), k0 < R0, by a product tree in fp32 (fft_core.hpp: twiddle_powers), in F1 and again in I3.  The
# rounding of the base is multiplied by k0: at 16384 points (R0 = 16) the powers are up to 8 eps off where a rounded
# table is 0.3 eps off (tests/test_fastfir_bins_host.py models it: the same block goes from 1.0 to 3.1 T_y).  Measured on the
# MI355X: at most 3.16 B_y and 4.28 T_y (wide filter), against 2.8 for the pipelined kernels; the margin is 1.5 x 4.28.
# At 8192 points and below (R0 <= 8) the kernel stays inside the common margin.  keys: (size, FastFirKernel)
MARGINS = {(16384, 0): 6.43}
SIZES = (2048, 4096, 8192, 16384)
FILTERS = [(-250, 250, 700, 48000.0), (300, 2700, -800, 48000.0), (-2800, -100, 0, 48000.0),
           (-5000, 5000, 0, 62500.0), (-0.49 * 62500, 0.49 * 62500, 0, 62500.0)]
NARROW, TEN_KHZ, WIDE = FILTERS[0], FILTERS[3], FILTERS[4]


def margin(n, kernel):
    """the factor over the yardstick that `kernel` (FastFirKernel: 0 generic, 1 pipelined on complex H, 2 on real gains) is held to"""
    return MARGINS.get((n, kernel), MARGIN)


def probe(n, seed):
    """one period: flat magnitude, random phases, 3000 rms (crest factor 3 to 3.3: the peak stays inside int16), complex64"""
    phi = np.random.default_rng(seed).uniform(0.0, 2.0 * np.pi, n)
    p = np.fft.ifft(np.exp(1j * phi))
    p *= RMS / np.sqrt(np.mean(np.abs(p) ** 2))
    return p.astype(np.complex64)


def stream(n, seed, periods=PERIODS):
    return np.tile(probe(n, seed), periods)


def rms(x):
    return float(np.sqrt(np.mean(np.abs(np.asarray(x, dtype=np.complex128)) ** 2)))


def spectrum(x, n):
    """X: the fp64 spectrum of the period the stream repeats (the complex64 words widened)"""
    return np.fft.fft(np.asarray(x[n:2 * n], dtype=np.complex128))


def _figures(e, X, g, xrms):
    E = np.fft.fft(e)
    return float((np.abs(E) / (np.abs(X) * g)).max()), float(np.abs(e).max() / (g * xrms))


def figures(got, ref, x, n, window=1):
    """(B, T) of `got` against `ref` on output samples [window n, (window + 1) n) of the stream x"""
    assert window >= 1 and len(ref) >= (window + 1) * n and len(got) >= (window + 1) * n
    sl = slice(window * n, (window + 1) * n)
    X = spectrum(x, n)
    r = np.asarray(ref[sl], dtype=np.complex128)
    g = float(np.abs(np.fft.fft(r) / X).max())
    return _figures(np.asarray(got[sl], dtype=np.complex128) - r, X, g, rms(x[n:2 * n]))


def effective_response(ref, x, n):
    """what the oracle multiplied every bin of the probe by (window 1), rounded to complex64"""
    return (np.fft.fft(np.asarray(ref[n:2 * n], dtype=np.complex128)) / spectrum(x, n)).astype(np.complex64)


def fp32_pair(ref, x, n, fault=None):
    """(y32, y64): one period through scipy's fp32 transform pair on Heff32, and the fp64 product on the same multipliers.
    fault(H) -> H changes the multipliers of the fp32 side only (the tests of the instrument plant single-bin faults)"""
    H32 = effective_response(ref, x, n)
    p32 = np.ascontiguousarray(x[n:2 * n], dtype=np.complex64)
    Hf = H32 if fault is None else np.asarray(fault(H32.copy()), dtype=np.complex64)
    y32 = scipy.fft.ifft(scipy.fft.fft(p32) * Hf)
    assert y32.dtype == np.complex64, y32.dtype              # (numpy.fft upcasts on older numpy; scipy.fft does not)
    y64 = np.fft.ifft(np.fft.fft(p32.astype(np.complex128)) * H32.astype(np.complex128))
    return y32, y64


def pair_figures(y32, y64, x, n):
    X = spectrum(x, n)
    g = float(np.abs(np.fft.fft(y64) / X).max())
    return _figures(y32.astype(np.complex128) - y64, X, g, rms(x[n:2 * n]))


def yardstick(ref, x, n):
    """(B_y, T_y): the figures of the plain fp32 transform pair for this stream and this filter; deterministic"""
    return pair_figures(*fp32_pair(ref, x, n), x, n)


def oracle_reference(oracle, n, x, cut):
    """the fp64 oracle on the widened complex64 words of x, fed in one call"""
    ff = oracle.CFastFIR(n)
    assert ff.SetupParameters(*cut) == 1
    ref = ff.ProcessData(np.asarray(x, dtype=np.complex128))
    assert len(ref) == len(x)
    return ref
