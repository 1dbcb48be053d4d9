"""The instrument of k3_bins.py on the CPU (no GPU): the fp32 yardstick of the display spectrum holds the rule it sets for
the kernels, at all eight sizes; faults planted on the yardstick's side -- one bin's amplitude 1e-4 off, one window
entry read one place off, two neighbouring display bins swapped, one frame missing from the mean -- are rejected; and
the gap this rule closes is on record: assert_spectrum_close (tests/test_fft_resampler_gpu.py), until now the only
numerical check behind every display path, accepts the first two."""
import functools

import numpy as np
import pytest

import k3_bins as K
from test_fft_resampler_gpu import assert_spectrum_close

CASES = [(1, 1), (3, 7)]                                 # (ave, frames): one frame alone; warm-up, then four frames of the exponential phase


@pytest.fixture(scope="module")
def orc(oracle):
    return oracle


@functools.lru_cache(maxsize=None)
def _case(n, ave, nframes, row):
    from oracle import oracle as orc
    orc.build()
    x = K.frames(n, 1, nframes, case=row)[0]
    ref, e_y = K.reference(orc, x, ave)
    ref.setflags(write=False)
    return x, ref, e_y


def yard(x, ave, **faults):
    y = K.Yard32(x.shape[1], ave, **faults)
    K.feed((y,), x)
    return y.ave_buf()


# ---- the yardstick holds its own rule
@pytest.mark.parametrize("ave,nframes", CASES)
@pytest.mark.parametrize("n", K.SIZES)
def test_yardstick_holds_its_own_rule(orc, n, ave, nframes):
    x, ref, e_y = _case(n, ave, nframes, 0)
    _, ref_b, e_y_b = _case(n, ave, nframes, 1)
    assert 0 < e_y < 1e-5 and 0 < e_y_b < 1e-5, (e_y, e_y_b)
    got = yard(x, ave)
    assert K.figure(got, ref, n) == e_y                                  # m = 1: deterministic
    print("yardstick n=%d ave=%d: E_y = %.3g, another seed's %.3g (ratio %.2f)" % (n, ave, e_y, e_y_b, e_y / e_y_b))
    assert K.check(got, ref, e_y_b, n, "yardstick, other seed's E_y") <= K.margin(n)
    assert e_y_b <= K.margin(n) * e_y


# ---- no skipped bins
@pytest.mark.parametrize("ave,nframes", CASES)
@pytest.mark.parametrize("n", K.SIZES)
def test_no_bin_is_left_out(orc, n, ave, nframes):
    """the clamp of the decode touches no bin of the oracle's output, and the weakest bin still decodes far above K_C"""
    _, ref, _ = _case(n, ave, nframes, 0)
    kb, kc = K.consts(n)
    p = 10.0 ** (ref - kb) - kc
    assert p.shape == (n,) and (p > 0.0).all()
    assert p.min() > 1e6 * kc, (p.min(), kc)
    assert (K.decode(ref, n, reference=True) > 0.0).all()


# ---- planted faults
def plant_amplitude(bels, n, ref, rel=1e-4):
    """one bin, its reference amplitude at least the rms one, rel off in amplitude; -> (bels, bin)"""
    a = K.decode(ref, n, reference=True)
    j = int(np.flatnonzero(a >= np.sqrt(np.mean(a ** 2)))[n // 7 % 50])
    kb, kc = K.consts(n)
    out = np.array(bels, dtype=np.float32)
    out[j] = np.float32(np.log10((a[j] * (1.0 + rel)) ** 2 + kc) + kb)
    return out, j


def rejected(got, ref, e_y, n):
    with pytest.raises(AssertionError):
        K.check(got, ref, e_y, n, "planted")
    return K.figure(got, ref, n) / e_y


@pytest.mark.parametrize("ave,nframes", CASES)
@pytest.mark.parametrize("n", [512, 4096, 65536])
def test_one_bin_amplitude_fault_is_rejected_and_was_accepted(orc, n, ave, nframes):
    x, ref, e_y = _case(n, ave, nframes, 0)
    bad, j = plant_amplitude(yard(x, ave), n, ref)
    r = rejected(bad, ref, e_y, n)
    print("one bin 1e-4 off (bin %d) n=%d ave=%d: %.1f E_y" % (j, n, ave, r))
    assert r > 2 * K.margin(n)
    assert_spectrum_close(bad.astype(np.float64), ref)                   # the gap on record: the old rule accepts it


@pytest.mark.parametrize("ave,nframes", CASES)
def test_window_entry_fault_is_rejected_and_was_accepted(orc, ave, nframes):
    """The new rule rejects it in both cases (197 and 146 E_y).  The old rule accepts it where the spectrum is averaged
    (ave 3, 7 frames: every bin within 0.001 bel); on ONE frame of the probe it objects, but only in a Rayleigh null of
    the probe (0.027 bel in one bin of 512, the typical bin 0.0004 bel off): its acceptance is asserted for the averaged
    case only."""
    n = 512
    x, ref, e_y = _case(n, ave, nframes, 0)

    def shifted(w):
        w[n // 4] = w[n // 4 + 1]
        return w
    bad = yard(x, ave, win_fault=shifted)
    r = rejected(bad, ref, e_y, n)
    print("window entry n/4 read one place off, n=%d ave=%d: %.1f E_y" % (n, ave, r))
    assert r > 2 * K.margin(n)
    if ave > 1:
        assert_spectrum_close(bad.astype(np.float64), ref)               # the gap on record: the old rule accepts it


@pytest.mark.parametrize("ave,nframes", CASES)
@pytest.mark.parametrize("n", [512, 2048, 32768])
def test_swapped_neighbours_are_rejected(orc, n, ave, nframes):
    x, ref, e_y = _case(n, ave, nframes, 0)
    bad = yard(x, ave)
    a = K.decode(ref, n)
    j = int(np.argmax(np.abs(np.diff(a))[:n // 2])) if n == 512 else n // 2 + 37     # any pair: neighbours differ like strangers
    bad[[j, j + 1]] = bad[[j + 1, j]]
    r = rejected(bad, ref, e_y, n)
    print("display bins %d, %d swapped, n=%d ave=%d: %.3g E_y" % (j, j + 1, n, ave, r))
    assert r > 100 * K.margin(n)


@pytest.mark.parametrize("n", [512, 8192])
def test_missing_frame_is_rejected(orc, n):
    """ave 3, frame 5 of 7 adds nothing to the running sum"""
    x, ref, e_y = _case(n, 3, 7, 0)
    bad = yard(x, 3, power_fault=lambda p, k: p * np.float32(0.0) if k == 5 else p)
    r = rejected(bad, ref, e_y, n)
    print("frame 5 of 7 missing from the mean, n=%d: %.3g E_y" % (n, r))
    assert r > 100 * K.margin(n)


def test_db_compensation_moves_the_constants(orc):
    """K_B and K_C follow the compensation: the yardstick and the decode with it set, against the oracle"""
    n, dbc = 1024, -6.0
    x = K.frames(n, 1, 2, case=2)[0]
    ref, e_y = K.reference(orc, x, 2, dbc)
    ref0, _ = K.reference(orc, x, 2)
    assert np.abs((ref - ref0) - dbc / 10.0).max() < 1e-6
    assert 0 < e_y < 1e-5
    assert np.allclose(K.decode(ref, n, dbc), K.decode(ref0, n), rtol=1e-9)
