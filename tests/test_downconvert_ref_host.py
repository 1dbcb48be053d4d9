"""The fp64 reference of the NCO + decimator cascade (tests/dc_ref.py) and the parity tolerance derived from it, proven
on the CPU: the reference does not depend on the chunking, agrees with the oracle's CDownConvert wherever the oracle
can run, the fp32 rounding floor of the stage formula over all 164 plans is at most K / 4, and -- what makes the
tolerance mean something -- zeroing ANY one tap pair of ANY stage of ANY plan, or moving its centre tap by one sample,
moves the reference by at least 2 K rms on the very inputs the GPU parity cases use."""
import numpy as np
import pytest

import dc_ref as D
import indep_ref as ind
from cutesdr_amd import _build

PLANS = _build.all_dc_plans()
NINE = (3, 3, 11, 11, 11, 11, 15, 23, 47)        # nine stages, CICs and short and long half bands
assert NINE in PLANS
CUT_PLANS = [(), (3,), (51,), (11, 11, 15, 19, 31), NINE]


def _pair(plan):
    return PLANS[plan] if plan else (2e6, 1e9)


def test_all_plans_are_164_and_cover_every_kind_in_every_position_checked():
    assert len(PLANS) == 164
    assert {p[-1] for p in PLANS} == set(D.KINDS)                  # every kind ends some plan
    inner = {k for p in PLANS for k in p[:-1]}
    assert {11, 15, 19} <= inner
    for k in D.KINDS:
        assert (k,) in PLANS                                       # the impulse cases' single-stage plans


@pytest.mark.parametrize("plan", CUT_PLANS)
def test_reference_does_not_depend_on_the_chunking(plan):
    """Within 1e-12 of the output rms, not bit-equal: the phase anchors sit on the absolute sample grid, so the mixed
    samples are the same words however the stream is cut, but upfirdn's sums over [history | input] are not promised to
    associate the same way at a call's start as in its middle."""
    rate, _ = _pair(plan)
    u = max(2, 1 << len(plan))
    rng = np.random.default_rng(7)
    calls = [int(rng.integers(1, 40)) * u for _ in range(30)]
    x = D.white(99, sum(calls))
    for first in (0, 300 - 300 % u, (1 << 32) - 4 * u):
        whole = D.dc_reference(plan, 0.123 * rate, rate, x, first_sample=first)
        cut = D.dc_reference(plan, 0.123 * rate, rate, x, first_sample=first, calls=calls)
        assert len(whole) == len(cut) == len(x) >> len(plan)
        assert np.abs(whole - cut).max() <= 1e-12 * D.rms(whole)


def test_late_phase_is_exact_and_first_sample_continues_a_stream():
    from fractions import Fraction
    rate, freq, first = 2.0 ** 21, 2.0 ** 21 * (0.3125 + 2.0 ** -33 + 2.0 ** -45), (1 << 32) - 6
    got = D.DcRef((), freq, rate, first).mix(np.ones(12))
    for i in range(12):
        turns = (Fraction(freq) / Fraction(rate) * (first + i + 1)) % 1
        want = D.A_INF * np.exp(2j * np.pi * float(turns))
        assert abs(got[i] - want) <= 1e-14
    # a stream entered late equals the stream run from its start, once the stage histories have filled
    plan = (11, 11, 15, 19, 31)
    x = D.white(5, 8192)
    full = D.dc_reference(plan, 0.21 * 2e6, 2e6, x)
    late = D.dc_reference(plan, 0.21 * 2e6, 2e6, x[2048:], first_sample=2048)
    w = D.warmup_len(plan) >> 5
    assert np.abs(full[(2048 >> 5) + w:] - late[w:]).max() <= 1e-12 * D.rms(full)
    # and a retune keeps the phasor: only the increment changes
    r = D.DcRef((), 1000.0, 2e6)
    a = r.mix(np.ones(700)); r.set_frequency(-3000.0); b = r.mix(np.ones(4))
    step = np.exp(-2j * np.pi * 3000.0 / 2e6)
    assert abs(b[0] - a[-1] * step) <= 1e-13 and abs(b[3] - a[-1] * step ** 4) <= 1e-13


def test_envelope_and_warmup_rule():
    e = D.envelope()
    assert e[0] == 1.0 and abs(e[1] - 0.95) < 1e-15 and abs(e[-1] - D.A_INF) < 1e-15
    assert D.warmup_len(()) == 0 and D.warmup_len((51,)) == 512
    assert D.warmup_len((11, 11, 15, 19, 31)) == 1024              # 10 + 20 + 56 + 144 + 480 = 710
    assert D.warmup_len(NINE) % 512 == 0 and D.warmup_len(NINE) >= sum(D.hist_of(k) << s for s, k in enumerate(NINE))


def test_reference_equals_the_oracle_on_every_plan_the_oracle_can_take(oracle):
    """Host-sized calls: a half-band stage must see at least 2 (taps - 1) samples per call (its in-place history copy,
    downconvert.cpp:314-317) and at most 32768 - (taps - 1) (its scratch buffer, :54).  Two calls of the largest
    multiple of 2^stages below 32000 satisfy both for all 164 plans and the pure mixer: none is left out."""
    worst = 0.0
    for plan in [()] + sorted(PLANS):
        rate, bw = _pair(plan)
        n_call = (32000 >> len(plan)) << len(plan)
        assert all(2 * D.hist_of(k) <= (n_call >> s) <= 32768 - D.hist_of(k) for s, k in enumerate(plan))
        dc = oracle.CDownConvert()
        dc.SetDataRate(rate, bw)
        assert tuple(dc.stages()) == plan
        f = D.parity_freq(rate)
        dc.SetFrequency(f)
        x = D.white(D.plan_seed(plan), 2 * n_call)
        want = np.concatenate([dc.ProcessData(x[:n_call]), dc.ProcessData(x[n_call:])])
        got = D.dc_reference(plan, f, rate, x)
        assert len(got) == len(want)
        err = np.abs(got - want).max() / D.rms(want)
        worst = max(worst, err)
        assert err <= 1e-9, plan
    print("dc_reference vs oracle, worst max|diff| / rms over %d plans: %.3g" % (len(PLANS) + 1, worst))


def test_fp32_floor_of_the_stage_formula_is_a_quarter_of_K():
    floors = {}
    for plan, (rate, _) in PLANS.items():
        x, f = D.parity_input(plan), D.parity_freq(rate)
        assert np.abs(x.real).max() > 0.99 * D.FULL_SCALE and np.abs(x.imag).max() > 0.99 * D.FULL_SCALE
        ref = D.dc_reference(plan, f, rate, x)
        m = D.dc_reference_fp32(plan, f, rate, x)
        floors[plan] = np.abs(m - ref)[1:].max() / D.rms(ref)
    worst = max(floors, key=floors.get)
    print("fp32 floor over %d plans: max|fp32 - fp64| / rms = %.4g at %s; K = %.3g" % (len(floors), floors[worst], worst, D.K))
    assert len(floors) == 164
    assert floors[worst] <= D.K / 4
    assert floors[worst] >= D.K / 8                                # K is four times the floor, not a loose round figure


def test_any_zeroed_tap_pair_or_moved_centre_exceeds_twice_the_tolerance():
    """Every plan, every stage, every pair (4127 mutations), on the GPU parity cases' own inputs and compared span
    (everything after the first output).  No plan is left out."""
    smallest, count = (np.inf, None), 0
    last_kinds, inner_kinds = set(), set()
    for plan, (rate, _) in PLANS.items():
        x, f = D.parity_input(plan), D.parity_freq(rate)
        ys = D.stage_inputs(plan, f, rate, x)
        ref = ys[-1]
        tol = D.tolerance(ref)
        assert np.abs(ref - D.dc_reference(plan, f, rate, x, calls=D.parity_calls(plan))).max() <= 1e-12 * D.rms(ref)
        for s, kind in enumerate(plan):
            (last_kinds if s + 1 == len(plan) else inner_kinds).add(kind)
            muts = [("pair %d" % q, D.mutate_pair(kind, q)) for q in range(D.n_pairs(kind))] + [("centre", D.mutate_centre(kind))]
            for name, h in muts:
                y = ind.DecimateBy2(h).run(ys[s])
                for k in plan[s + 1:]:
                    y = ind.DecimateBy2(D.stage_taps(k)).run(y)
                d = np.abs(y - ref)[1:].max()
                assert d >= 2 * tol, (plan, s, name, d / D.rms(ref))
                count += 1
                if d / D.rms(ref) < smallest[0]:
                    smallest = (d / D.rms(ref), (plan, s, name))
    assert last_kinds == set(D.KINDS) and {11, 15, 19} <= inner_kinds
    print("%d mutations; smallest max|mutated - ref| / rms = %.3g (%.1f K) at %s" % (count, smallest[0], smallest[0] / D.K, smallest[1]))


def test_mutations_through_the_taps_argument_match_the_stage_wise_shortcut():
    plan, (rate, _) = (11, 15, 23, 51), PLANS[(11, 15, 23, 51)]
    x, f = D.parity_input(plan), D.parity_freq(rate)
    ys = D.stage_inputs(plan, f, rate, x)
    h = D.mutate_pair(51, 0)
    assert h[0] == 0.0 and h[50] == 0.0 and h[2] != 0.0 and h[25] == 0.5
    a = D.dc_reference(plan, f, rate, x, taps={3: h})
    b = ind.DecimateBy2(h).run(ys[3])
    assert np.array_equal(a, b)
    c = D.mutate_centre(51)
    assert c[25] == 0.0 and c[26] == 0.5 + D.HB_EVEN[51][12] and abs(c.sum() - D.stage_taps(51).sum()) < 1e-15
    assert list(D.mutate_pair(3, 0) * 8) == [0, 3, 3, 0] and list(D.mutate_centre(3) * 8) == [3, 1, 1, 3]


@pytest.mark.parametrize("kind", D.KINDS)
def test_impulse_expectation_is_the_reference(kind):
    """the expectation of the GPU impulse cases (taps written out by index) against dc_reference; expected zeros exact"""
    rate, _ = PLANS[(kind,)]
    for n in (2048, 1936):
        want = D.impulse_expected(kind, n)
        ref = D.dc_reference((kind,), 0.0, rate, D.impulse_input(n))
        assert np.abs(want - ref).max() <= 1e-12 * D.FULL_SCALE
        nz = np.flatnonzero(want)
        # the even-index impulse meets the even taps (every pair, both ends), the odd-index one the centre alone
        assert len(nz) == (4 if kind == 3 else 2 * D.n_pairs(kind) + 1)
        assert np.all(ref[want == 0] == 0)
