"""The K9 word rule: the batch signal generator's output words (testgen_kernels.hip) against the exact phase of the
restatement's own frequency sequence.  Nothing here calls the library; DESIGN.md section 6 has the rule in prose.

For one receiver's stream the restatement (testgen_ref.RefTestBench, driven in 256-sample calls with trace=) gives the
bit-exact frequency sequence, the gate, the amplitude in force and the noise terms g1, g2.  The phase theta_j in turns is
the exact rational sum of that sequence over Fs (exact_turns' construction, at every sample), restarted at 0 wherever the
restatement sets m_SweepAcc = 0.0 (the sweep slots, Reset, a rate change); cos and sin of 2 pi theta are taken in
numpy.longdouble from a hi + lo pair of the fraction.

    centre      y = amp cos(2 pi theta) + namp g1, the imaginary part with sin and g2; real overload 3 amp cos + namp g1
    half width  d = amp' PHI + namp |g| 2^-49          (amp' = amp, or 3 amp in the real form; amp = 0 with the gate closed)
    words       lo = fp32(y - d), hi = fp32(y + d), round to nearest; lo == hi: the word is decided and the device word
                equals it as a value (-0.0 == +0.0); otherwise lo <= word <= hi
    cap         per row and component at most CAP of the gate-open words undecided (a condition on the inputs, checked
                from the reference alone in test_testgen_words_host.py)

PHI = 4.0e-10 rad is derived from the kernel's stated arithmetic, not measured:
    the phase is read in units of 2^-34 turn (truncated)            2 pi 2^-34 = 3.66e-10 rad
    truncation of the two Taylor polynomials at +-pi/4              7e-12
    the host's 128-bit phase against the exact one                  1.5e-12 (test_testgen_host.py's bound)
    fp64 roundings (argument, polynomials, product, sum)            the rest, 2.5e-11
The noise term allows 16 fp64 ulps (2^-49) for log, the division, sqrt and the products.
"""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

import testgen_ref as R

LD = np.longdouble
PHI = 4.0e-10
NOISE_REL = 2.0 ** -49
CAP = 0.08
CALL = 256                                # the restatement's call length: the yardstick of the K9 tests
TWO_PI_LD = LD(6.283185307179586) + LD(2.4492935982947064e-16)       # 2 pi as a double-double, summed in 64 bits
SHIFT = 1200                              # every fp64 frequency is an integer multiple of 2^-SHIFT
RESTART_SLOTS = ("OnSweepStart", "OnSweepStop", "OnSweepRate", "Reset")


# ---------------------------------------------------------------------------------------------- exact phase
def _mantissas(freq):
    m, e = np.frexp(np.asarray(freq, dtype=np.float64))
    return (m * 2.0 ** 53).astype(np.int64), e


def exact_turns(freq, fs, at):
    """exact phase in turns (Fraction, modulo 1) before samples `at` of the frequency sequence freq over fs"""
    mant, e = _mantissas(freq)
    s, out, at = 0, {}, set(int(a) for a in at)
    for j in range(len(freq) + 1):
        if j in at:
            t = Fraction(s, 1 << SHIFT) / Fraction(fs)
            out[j] = t - math.floor(t)
        if j < len(freq):
            s += int(mant[j]) << (int(e[j]) - 53 + SHIFT)
    return out


def exact_turns_all(freq, fs):
    """the same phase before every sample 0..len(freq)-1 as (hi, lo) longdoubles: hi + lo is the fraction of a turn
    truncated to 2^-128"""
    mant, e = _mantissas(freq)
    fr = Fraction(fs)
    q, M = fr.denominator, fr.numerator << SHIFT
    n = len(freq)
    limbs = np.zeros((n, 4), dtype=np.uint64)
    s = 0
    for j in range(n):
        t = (((s * q) % M) << 128) // M
        limbs[j] = ((t >> 96) & 0xFFFFFFFF, (t >> 64) & 0xFFFFFFFF, (t >> 32) & 0xFFFFFFFF, t & 0xFFFFFFFF)
        s += int(mant[j]) << (int(e[j]) - 53 + SHIFT)
    w = limbs.astype(np.float64).astype(LD)                          # 32-bit limbs: exact in every step
    hi = w[:, 0] * LD(2.0) ** -32 + w[:, 1] * LD(2.0) ** -64
    lo = w[:, 2] * LD(2.0) ** -96 + w[:, 3] * LD(2.0) ** -128
    return hi, lo


def cos_sin_turns(hi, lo):
    a = TWO_PI_LD * hi + TWO_PI_LD * lo
    return np.cos(a), np.sin(a)


# ---------------------------------------------------------------------------------------------- the streams
class Plan:
    """receivers (testgen_ref.RECEIVERS' tuples), their noise powers (None: off), the seed and the sections of the
    stream: (samples, rate, [(receiver, slot, value) called before the section])"""

    def __init__(self, name, receivers, noise, seed, sections):
        self.name, self.receivers, self.noise, self.seed, self.sections = name, receivers, noise, seed, sections
        self.n = sum(s[0] for s in sections)
        assert len(noise) == len(receivers) and all(s[0] % CALL == 0 for s in sections)

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self is other


FS1, FS2 = R.FS1, R.FS2
N = 8192
# (start Hz, stop Hz, rate Hz/s, width s, period s, signal dB, on); at 2 MSPS one sample is 5e-7 s
RECEIVERS = [
    (123456.789, 123456.789, 0.0, 0.0, 0.5, 0.0, True),            # 0 full-scale tone
    (937123.5, 937123.5, 0.0, 0.0, 0.5, 0.0, True),                # 1 tone near Fs/2
    (-271828.18, -271828.18, 0.0, 0.0, 0.5, -60.0, True),          # 2 -60 dB tone
    (10007.3, 10007.3, 0.0, 0.0, 0.5, -160.0, True),               # 3 -160 dB tone: 3.3e-4 counts
    (-3000.0, 3000.0, 3.3e6, 0.0, 0.5, 0.0, True),                 # 4 through zero, 1.65 Hz a sample, ends at 3637
    (100000.5, 130000.25, 2.0e7, 0.0, 0.5, 0.0, True),             # 5 a sweep that ends inside the stream (3000)
    (213377.3, 100000.0, 1.0e6, 0.0, 0.5, 0.0, True),              # 6 start >= stop: one step, then constant
    (263171.7, 263171.7, 0.0, 3.4e-6, 4.97e-5, 0.0, True),         # 7 pulse: 7 samples in 100
    (-500000.0, -100000.0, 7.7e7, 1.02e-5, 5.02e-5, -6.0, True),   # 8 pulsed sweep: 21 samples in 101
    (-241899.9, -241899.9, 0.0, 0.2, 1.0e-4, 0.0, True),           # 9 width >= period: the timer runs, the gate stays open
    (31250.3, 31250.3, 0.0, 5.124e-4, 0.5, 0.0, True),             # 10 a period never reached; the gate closes at 1024
    (55555.0, 66666.0, 1000.0, 0.001, 0.1, 0.0, False),            # 11 OFF: its row stays as it was
    (1000.1, 300000.0, 5.0e5, 0.0, 0.5, 0.0, True),                # 12 OnSweepStart / OnSweepStop between calls
    (0.0, 20000.0, 1.0e7, 0.0, 0.5, 0.0, True),                    # 13 OnSweepRate re-arms the sweep, which then ends
    (41250.7, 41250.7, 0.0, 3.0e-4, 1.0e-3, 0.0, True),            # 14 OnSignalPwr, OnPulseWidth, OnPulsePeriod, Reset
    (1777.7, 1777.7, 0.0, 0.0, 0.5, -20.0, True),                  # 15 switched off for one section
    (10007.3, 10007.3, 0.0, 1.02e-5, 5.02e-5, -160.0, True),       # 16 -160 dB behind a gate: 21 samples in 101
]
THROUGH_ZERO, OFF_ROW, GATED_TINY = 4, 11, 16
SECTIONS = [
    (2560, FS1, []),
    (1536, FS1, [(12, "OnSweepStart", -100000.3), (13, "OnSweepRate", 2.0e7), (14, "OnSignalPwr", -10.0),
                 (15, "OnGenOn", False)]),
    (1024, FS1, [(14, "OnPulseWidth", 1.0e-4), (14, "OnPulsePeriod", 2.5e-4), (14, "Reset", None),
                 (12, "OnSweepStop", 50000.0), (15, "OnGenOn", True), (5, "OnSweepRate", 3.3e6)]),
    (3072, FS2, [(9, "OnPulseWidth", 0.0)]),
]
MAIN = Plan("main", RECEIVERS, [None] * len(RECEIVERS), 0, SECTIONS)

NOISE_RECEIVERS = [
    (10007.3, 10007.3, 0.0, 0.0, 0.5, -160.0, True),               # 0 noise -70 dB
    (10007.3, 10007.3, 0.0, 0.0, 0.5, -160.0, True),               # 1 noise -20 dB
    (123456.789, 123456.789, 0.0, 0.0, 0.5, 0.0, True),            # 2 full-scale tone, noise -40 dB
    (263171.7, 263171.7, 0.0, 1.02e-5, 5.02e-5, 0.0, True),        # 3 the same behind a gate: noise alone when closed
]
NOISE_DB = [-70.0, -20.0, -40.0, -40.0]
NOISE_SECTIONS = [(4096, FS1, []), (1024, FS1, [(3, "OnSignalPwr", -6.0)]), (3072, FS2, [])]
NOISE_SEEDS = R.NOISE_SEEDS
NOISE = {seed: Plan("noise-%d" % seed, NOISE_RECEIVERS, NOISE_DB, seed, NOISE_SECTIONS) for seed in NOISE_SEEDS}
assert MAIN.n == N and all(p.n == N for p in NOISE.values())

CUTS = ("one", "256", "ragged")
RAGGED = [2, 6, 1022, 510, 333]           # then the rest of the section


def split(n, cut):
    if cut == "one":
        return [n]
    if cut == "256":
        return [CALL] * (n // CALL)
    out = []
    for m in RAGGED:
        if sum(out) + m >= n:
            break
        out.append(m)
    return out + [n - sum(out)]


def calls(plan, cut, q):
    """the calls of one cut: (events before the call, samples, rate, first sample of the stream, offset in the row,
    section).  q: samples per 16-byte store (2 complex, 4 real); a call that ends off a multiple of q leaves a gap, so
    that every row start stays 16-byte aligned.  Returns the list and the row length the cut needs."""
    out, pos, off = [], 0, 0
    for k, (n, fs, events) in enumerate(plan.sections):
        for i, m in enumerate(split(n, cut)):
            out.append((events if i == 0 else [], m, fs, pos, off, k))
            pos += m
            off = -(-(off + m) // q) * q
    return out, off


def positions(plan, cut, q):
    """row index of every sample of the stream, and each sample's index within its call"""
    where, jcall = np.zeros(plan.n, dtype=np.int64), np.zeros(plan.n, dtype=np.int64)
    for _, m, _, pos, off, _ in calls(plan, cut, q)[0]:
        where[pos:pos + m] = off + np.arange(m)
        jcall[pos:pos + m] = np.arange(m)
    return where, jcall


# ---------------------------------------------------------------------------------------------- the reference
@lru_cache(maxsize=None)
def reference(plan, c):
    """receiver c of a plan through the restatement in 256-sample calls: a dict of per-sample arrays
    on, gate, restart, fs, freq, amp (in force, gate or not), namp (0 with the noise off), g1, g2, cos, sin (longdouble,
    of the exact phase), ref (the restatement's complex128 output), ref_real (its real overload)"""
    n = plan.n
    r, rr = R.RefTestBench(seed=plan.seed, channel=c), R.RefTestBench(seed=plan.seed, channel=c)
    for o in (r, rr):
        R.configure(o, plan.receivers[c], noise_db=plan.noise[c])
    d = {k: np.zeros(n) for k in ("fs", "freq", "amp", "namp", "g1", "g2", "ref_real")}
    d.update({k: np.zeros(n, dtype=bool) for k in ("on", "gate", "restart")})
    d["ref"] = np.zeros(n, dtype=np.complex128)
    pos, restart = 0, True
    for m, fs, events in plan.sections:
        for rc, name, v in events:
            if rc == c:
                R.slot(r, name, v)
                R.slot(rr, name, v)
                restart |= name in RESTART_SLOTS
        for p in range(pos, pos + m, CALL):
            s = slice(p, p + CALL)
            if not r.m_GenOn:
                continue
            restart |= r.m_GenSampleRate != fs                          # create() resets before the first sample
            count, tr = r.count, {}
            d["ref"][s] = r.create(CALL, fs, trace=tr)
            d["ref_real"][s] = rr.create(CALL, fs, real=True)
            assert (tr["acc"][0] == 0.0) >= restart
            d["restart"][p], restart = restart, False
            d["on"][s], d["gate"][s], d["freq"][s], d["fs"][s] = True, tr["gate"], tr["freq"], fs
            d["amp"][s] = r.m_SignalAmplitude
            if r.m_NoisePower > -160.0:
                d["namp"][s] = r.m_NoiseAmplitude
                d["g1"][s], d["g2"][s], _ = R.gauss(plan.seed, c, count, CALL)
        pos += m
    on = np.nonzero(d["on"])[0]
    d["cos"], d["sin"] = np.ones(n, dtype=LD), np.zeros(n, dtype=LD)
    d["turns"] = np.zeros(n)
    starts = [i for i in on if d["restart"][i]]
    for a, b in zip(starts, starts[1:] + [n]):
        idx = on[(on >= a) & (on < b)]
        hi, lo = exact_turns_all(d["freq"][idx], float(d["fs"][a]))
        d["cos"][idx], d["sin"][idx] = cos_sin_turns(hi, lo)
        d["turns"][idx] = hi.astype(np.float64)
    for v in d.values():
        v.setflags(write=False)
    return d


def centre(d, real):
    """(y, delta) of a reference: longdouble, shape (n, 2) re / im, or (n, 1) for the real overload"""
    a = np.where(d["gate"], d["amp"], 0.0).astype(LD) * (3 if real else 1)
    namp = d["namp"].astype(LD)
    comps = [(d["cos"], d["g1"])] if real else [(d["cos"], d["g1"]), (d["sin"], d["g2"])]
    y = np.stack([a * t + namp * g.astype(LD) for t, g in comps], axis=1)
    delta = np.stack([a * LD(PHI) + namp * np.abs(g).astype(LD) * LD(NOISE_REL) for _, g in comps], axis=1)
    return y, delta


def interval(y, delta):
    return (y - delta).astype(np.float32), (y + delta).astype(np.float32)


def columns(x, real):
    """a stream of complex or real samples as (n, 2) / (n, 1) float64"""
    x = np.asarray(x)
    return x.astype(np.float64)[:, None] if real else np.stack([x.real, x.imag], axis=1).astype(np.float64)


def undecided_share(d, real):
    """per component: the share of the gate-open words of the row that the rule leaves undecided"""
    lo, hi = interval(*centre(d, real))
    m = d["on"] & d["gate"]
    return [float(np.mean(lo[m, k] != hi[m, k])) for k in range(lo.shape[1])]


class Tally:
    """one row (and form) under the rule; `got`: (n, 2) / (n, 1) values of the fp32 words"""

    def __init__(self, name, d, real, got):
        y, delta = centre(d, real)
        lo, hi = interval(y, delta)
        on = d["on"]
        got = np.asarray(got, dtype=np.float64)
        g32 = got.astype(np.float32)
        assert np.array_equal(g32.astype(np.float64)[on], got[on]), "fp32 words expected"
        inside = (g32 >= lo) & (g32 <= hi)                              # lo == hi: equality as values, -0.0 == +0.0
        decided = (lo == hi) & on[:, None]
        open_ = (on & d["gate"])[:, None] & np.ones_like(decided)
        self.name = name
        self.bad = int(np.count_nonzero(~inside & on[:, None]))
        self.first_bad = [(int(j), int(k), float(got[j, k]), float(lo[j, k]), float(hi[j, k]))
                          for j, k in np.argwhere(~inside & on[:, None])[:4]]
        self.decided = int(np.count_nonzero(decided))
        self.words = int(np.count_nonzero(on)) * lo.shape[1]
        self.open = int(np.count_nonzero(open_))
        self.share = float(np.count_nonzero(~decided & open_)) / max(1, self.open)
        nz = (delta > 0) & on[:, None]
        self.ratio = float((np.abs(got.astype(LD) - y)[nz] / delta[nz]).max()) if nz.any() else 0.0
        closed = (on & ~d["gate"] & (d["namp"] == 0.0))
        self.closed_zero = bool((got[closed] == 0.0).all())
        self.ok = self.bad == 0 and self.closed_zero

    def __str__(self):
        return ("%s: %d of %d words outside their interval; %d decided words compared, %.2f %% of the %d gate-open words "
                "undecided, largest |got - y| / delta %.3g%s" %
                (self.name, self.bad, self.words, self.decided, 100.0 * self.share, self.open, self.ratio,
                 "" if self.ok else "  FIRST " + repr(self.first_bad)))


# ---------------------------------------------------------------------------------------------- the old bounds
OLD_TOL = 1e-5 * R.MAX_AMPLITUDE          # test_testgen_gpu.py: 1e-5 of full scale, 3 x that for the real overload


def passes_old_bound(d, real, got):
    """the conditions of tests/test_testgen_gpu.py on one row: noise off |got - restatement| <= 1e-5 full scale (3 x in
    the real form); noise on <= 1e-5 namp max(1, |value| / namp)"""
    ref = columns(d["ref_real"] if real else d["ref"], real)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)[d["on"]]
    if (d["namp"] > 0).any():
        namp = d["namp"][d["on"]][:, None]
        return bool((err <= 1e-5 * namp * np.maximum(1.0, np.abs(ref[d["on"]]) / namp)).all())
    return bool((err <= (3.0 if real else 1.0) * OLD_TOL).all())
