"""The HIP path against the REFERENCE's own dsp/ code (oracle/ref.py -> oracle/_ref/libcutesdr_ref.so), directly: the
existing parity tests run unchanged -- same inputs, same assertions, same tolerances -- with the reference's compiled
classes as the checker instead of the fp64 oracle this project wrote.  The module-level fixture `oracle` below takes the
place of conftest.py's; everything imported from the other test modules sees oracle.ref through it.

Only the library is loaded here, never the reference tree (the GPU machine has none).  Skipped where the library is
absent.  Limits of this checker: the 2048-point filter only (CONV_FFT_SIZE is a constant of dsp/fastfir.cpp), no sound
sink, objects constructed into zeroed storage (oracle/ref.py)."""
import numpy as np
import pytest

import dc_ref as D
import test_postchain_gpu as TP
import test_fft_resampler_gpu as TF
import test_frontend_gpu as TN
import test_downconvert_plans_gpu as TD
from util_signals import tones_plus_noise

# run as they are, parametrisation included: the fixture `oracle` they ask for is this module's
from test_postchain_gpu import (test_agc_complex_and_real, test_smeter, test_am_sam_fm_demod_leaves,          # noqa: F401
                                test_leaf_objects_ragged_call_lengths, test_pll_unlockable_carrier_and_relock,
                                test_fir_design_and_filtering, test_iir_design_and_filtering,
                                test_cdemodulator_chain_reference_call_pattern)
from test_fft_resampler_gpu import test_resampler_all_overloads, test_resampler_rate_varies_per_call_like_the_sound_sink  # noqa: F401
from test_rate_change_gpu import test_dropin_input_rate_change_in_mid_stream                                  # noqa: F401

pytestmark = pytest.mark.gpu
TOL = 2e-5


@pytest.fixture(scope="module")
def oracle():
    from oracle import ref
    if ref.build() is None:
        pytest.skip("oracle/_ref/libcutesdr_ref.so is not here (it is built where the reference tree is)")
    return ref


# ------------------------------------------------------------------------------------------------ borrowed, a subset of sizes
@pytest.mark.parametrize("n,ave", [(512, 2), (4096, 1), (16384, 3), (65536, 1)])
def test_display_spectrum_matches_reference(oracle, n, ave):
    TF.test_display_spectrum_matches_oracle(oracle, n, ave)


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192, 16384, 32768, 65536])
def test_plain_transforms(oracle, n):
    TF.test_plain_transforms(oracle, n)


def test_demod_batch_mixed_modes_2048(oracle):
    """DemodBatch(6, 2048), AM / FM / USB / FM / SAM / LSB, two calls, under check_chain_bursts"""
    TP.test_demod_batch_mixed_modes(oracle, 2048)


# ------------------------------------------------------------------------------------------------ borrowed, the blanker
class _Front:
    """oracle.ref for the blanker tests, which hand over calls of up to 300 000 samples: CNoiseProc::ProcessBlanker
    holds 4096 (its test-bench buffer) and the binding refuses more, so the SAME stream goes in as pieces of 4096 -- the
    blanker's state carries from call to call, the output words are those of one long call.  The datagram unpacking
    is no part of dsp/ (interface/netiobase.cpp needs Qt's network classes): it only prepares the input of both sides
    and comes from the fp64 oracle."""

    def __init__(self, ref):
        from oracle import oracle as orc
        self._ref, self.unpack_packets = ref, orc.unpack_packets
        piece = ref.limit("BLANKER_CALL")

        class CNoiseProc(ref.CNoiseProc):
            def ProcessBlanker(self, x):
                out = [ref.CNoiseProc.ProcessBlanker(self, x[i:i + piece]) for i in range(0, len(x), piece)]
                return np.concatenate(out) if out else np.zeros(0, dtype=np.complex128)
        self.CNoiseProc = CNoiseProc

    def __getattr__(self, name):
        return getattr(self._ref, name)


@pytest.mark.parametrize("fs,thresh,width", [(2e6, 50.0, 2.0), (2e6, 20.0, 100.0), (500e3, 80.0, 3000.0), (6e6, 35.0, 10.0), (2e6, 40.0, 2040.0)])
def test_blanker_matches_reference_across_calls(oracle, fs, thresh, width):
    TN.test_blanker_matches_oracle_across_calls(_Front(oracle), fs, thresh, width)


@pytest.mark.parametrize("fs,width", [(2e6, 20.0), (2000200.0, 21.0), (500e3, 100.0), (6e6, 10.0), (2e6, 2040.0)],
                         ids=["ring-odd-lag", "ring-even-lag", "window-below-a-tile", "window-beyond-the-ring", "ring-widest-blank"])
@pytest.mark.parametrize("src", ["rows", 1028, 1444])
def test_blank_mask_is_bit_exact(oracle, src, fs, width):
    TN.test_blank_mask_is_bit_exact(_Front(oracle), src, fs, width)


# ------------------------------------------------------------------------------------------------ no test to borrow
CUTS = [(-5000, 5000, 0), (100, 2800, 0), (-2800, -100, 0), (-250, 250, 700)]       # test_batch_distinct_filters_and_response


def test_fastfir_batch_2048_against_the_reference_filter(oracle):
    """FastFirBatch(4, 2048) with four filters of its own: 5 hops through process within 2e-5 * max|x| of
    CFastFIR::ProcessData, response(c) within 1e-12 of the reference's m_pFilterCoef"""
    import cutesdr_amd as ca
    C, n, fs = 4, 2048, 62500.0
    T = 5 * (n // 2)
    x = np.stack([tones_plus_noise(c, T, fs, [500.0 * (c + 1), -12000.0]) for c in range(C)])
    b = ca.FastFirBatch(C, n)
    b.setup(-5000, 5000, 0, fs)
    for c, (lo, hi, off) in enumerate(CUTS):
        assert b.setup(lo, hi, off, fs, channel=c) == 1
    y = b.process(x)
    for c, (lo, hi, off) in enumerate(CUTS):
        ff = oracle.CFastFIR(n)
        ff.SetupParameters(lo, hi, off, fs)
        err_h = np.abs(b.response(c) - ff.coef()).max()
        ref = ff.ProcessData(x[c])
        assert len(ref) == T
        err = np.abs(y[c] - ref).max()
        print("REFDIRECT fastfir ch %d: response err %.3g, output err %.3g of max|x|" % (c, err_h, err / np.abs(x[c]).max()))
        np.testing.assert_allclose(b.response(c), ff.coef(), atol=1e-12)
        assert err <= TOL * np.abs(x[c]).max(), (c, err)


def test_device_designed_responses_against_the_reference(oracle):
    """The fp64 design that csdr_demod_batch_set_demod_many runs on the device (fastfir_design_kernels.hip, reached here
    through csdr_fastfir_batch_setup_many, which exposes the designed rows) for 8 receivers -- the four cuts above and the
    modes' default edges -- against the reference's m_pFilterCoef, held to 5e-16 * max|H|, the figure README.md gave
    for it.

    Measured on an MI355X: 2.2e-16 ... 4.6e-16 * max|H| over the eight filters.  The reference's own Ooura transform is
    1.9e-16 ... 4.2e-16 from a transform in 64-bit-mantissa arithmetic, so the bound leaves the design about one rounding
    of a pass-band word: it held only once the design kernel took a twiddle table of nearest doubles (host_math.hpp:
    design_twiddles; with the oracle's table, whose angles are rounded before cos / sin, it was 4.7e-16 ... 8.7e-16 and
    this test failed) and uncontracted butterflies, which a plain fp64 model reproduces (HISTORY.md)."""
    import cutesdr_amd as ca
    n, fs = 2048, 62500.0
    sets = [tuple(map(float, c)) for c in CUTS] + [(-5000.0, 5000.0, 0.0), (-3000.0, 3000.0, 0.0), (300.0, 2400.0, 0.0), (-300.0, 300.0, -700.0)]
    b = ca.FastFirBatch(len(sets), n)
    b.setup(-4000, 4000, 0, fs)
    st = b.setup_many(np.arange(len(sets)), [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets], fs)
    assert (st == 1).all(), st
    worst = 0.0
    for c, (lo, hi, off) in enumerate(sets):
        ff = oracle.CFastFIR(n)
        ff.SetupParameters(lo, hi, off, fs)
        want, got = ff.coef(), b.response(c)
        rel = np.abs(got - want).max() / np.abs(want).max()
        print("REFDIRECT device design %s: max err / max|H| %.3g" % ((lo, hi, off), rel))
        worst = max(worst, rel)
    assert worst <= 5e-16, worst


DC_PAIRS = [(2e6, 15000.0), (2e6, 1000.0), (10e6, 15000.0), (1.8e6, 20000.0), (500e3, 10000.0), TD.PLANS[TD.NINE]]


@pytest.mark.parametrize("rate,bw", DC_PAIRS, ids=lambda v: "%g" % v)
def test_downconverter_against_the_reference(oracle, rate, bw):
    """run_host_form / assert_parity of tests/test_downconvert_plans_gpu.py, 3 calls of 8192 samples with a retune in
    front of the third, the reference's CDownConvert given the same calls.  The nine-stage plan gets calls of 32768: a
    reference half band fed fewer than 2 (taps - 1) samples takes its history from data it has already overwritten, and
    fed fewer than `taps` it skips the call (downconvert.cpp:291-292, 314-317; DESIGN.md: the library keeps filtering,
    on purpose) -- 8192 samples leave the 47-tap ninth stage 32."""
    r = oracle.CDownConvert()
    assert r.SetDataRate(rate, bw) == rate / (1 << len(r.stages()))
    plan = tuple(int(s) for s in r.stages())
    need = max([2 * (L - 1) << i for i, L in enumerate(plan) if L not in (3, 11)] + [0])
    n = 8192 if need <= 8192 else 32768
    assert need <= n and (n == 8192 or plan == TD.NINE)
    calls, f1, f2 = [n, n, n], 0.0617 * rate, -0.21 * rate
    x = D.white(4100 + len(plan), sum(calls))
    got = TD.run_host_form(plan, f1, x, calls, retunes={2: f2}, pair=(rate, bw))
    r.SetFrequency(f1)
    ref = []
    for i in range(3):
        if i == 2:
            r.SetFrequency(f2)
        ref.append(r.ProcessData(x[i * n:(i + 1) * n].astype(np.complex128)))
    TD.assert_parity(got, np.concatenate(ref), "reference %s" % "-".join(map(str, plan)))
