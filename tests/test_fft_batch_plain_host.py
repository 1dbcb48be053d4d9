"""The references of the batch plain transforms hold on their own (no GPU): for all eight sizes and both signs the fp64
oracle's CFft::FwdFFT / RevFFT agrees with numpy's fp64 transform to 1e-12 sqrt(n) rms -- and, where the reference's own
code is built (oracle/_ref), with the reference's CFft --, and the yardstick of fft_plain_ref.py (scipy's fp32 transform)
stays finite and below 1e-6, far inside the rule it sets for the kernels."""
import numpy as np
import pytest

import fft_plain_ref as P


def numpy_fft(x, sign):
    x = np.asarray(x, dtype=np.complex128)
    return np.fft.ifft(x) * len(x) if sign > 0 else np.fft.fft(x)


@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", P.SIZES)
def test_oracle_agrees_with_numpy_and_the_yardstick_is_small(n, sign):
    seed = P.seed_of(n, 0)
    x = P.probe(n, seed)
    ref, e_y = P.reference(n, seed, sign)
    assert ref.dtype == np.complex128 and len(ref) == n
    assert np.abs(ref - numpy_fft(x, sign)).max() <= 1e-12 * np.sqrt(n) * P.RMS
    assert np.isfinite(e_y) and 0 < e_y < 1e-6, e_y
    # the probe is what the measure assumes: every bin of its transform has magnitude sqrt(n) rms (to complex64 rounding)
    assert np.abs(np.abs(ref) / (np.sqrt(n) * P.k1_bins.rms(x)) - 1).max() < 1e-5


@pytest.mark.parametrize("sign", P.SIGNS)
@pytest.mark.parametrize("n", P.SIZES)
def test_oracle_agrees_with_the_reference_code(n, sign):
    from oracle import ref as oref
    if not oref.available():
        pytest.skip("oracle/_ref is not built")
    seed = P.seed_of(n, 0)
    x = P.probe(n, seed)
    ref, _ = P.reference(n, seed, sign)
    got = oref.fft(x.astype(np.complex128), sign)
    assert np.abs(got - ref).max() <= 1e-12 * np.sqrt(n) * P.RMS


@pytest.mark.parametrize("sign", P.SIGNS)
def test_impulse_reference(sign):
    """the closed form the index-order test compares against is the transform of an impulse"""
    n, m = 512, 259
    x = np.zeros(n, dtype=np.complex128)
    x[m] = 3000.0
    assert np.abs(P.impulse_ref(n, m, sign) - numpy_fft(x, sign)).max() <= 1e-9 * 3000.0


def test_the_measure_sees_a_swapped_bin_pair_and_a_conjugate():
    """a permuted or conjugated spectrum is far outside the rule"""
    n = 1024
    seed = P.seed_of(n, 0)
    ref, e_y = P.reference(n, seed, +1)
    bad = ref.copy()
    bad[[5, 6]] = bad[[6, 5]]
    assert P.rel_err(bad, ref, P.probe(n, seed)) > 1000 * P.margin(n) * e_y
    with pytest.raises(AssertionError):
        P.check_frame(np.conj(ref), n, seed, +1)
    assert P.check_frame(P.yard_fft(P.probe(n, seed), +1), n, seed, +1) == pytest.approx(1.0)
