"""The NCO + decimator cascade (K2) in fp64, any plan, any chunking, any stream position -- TEST INFRASTRUCTURE.

Built on tests/indep_ref.py: the start-up envelope is `nco_mix` at 0 Hz (the amplitude recurrence of the first 512
samples), every stage one `DecimateBy2` (scipy.signal.upfirdn on [history | input]) with the taps of
include/csdr_hb_taps.h.  Behind sample 512 the amplitude is the settled sqrt(0.95) and the phase of sample n is
(n + 1) * freq / rate mod 1 taken EXACTLY (fractions.Fraction of the two doubles) at an anchor every 4096 samples on
the absolute sample grid and as a short split product inside (exact high part, < 2^-50 turns of error), so a stream that starts at sample
2^32 is as accurate as one that starts at 0.  Nothing here is imported by the product.

`dc_reference_fp32` is the same formula evaluated in fp32 with numpy: a model of "any honest fp32 evaluation", written
from the stage formula in the header comment of downconv_kernel.hpp (y[j] = sum_k h[k] xe[2j+k]; centre product first,
then the pairs in tap order), not from the kernel's code.  It exists to measure the rounding floor, from which the
parity tolerance `tol = K * rms(reference)` is derived (DESIGN.md, K2 parity rule).
"""
import math
import os
import re
from fractions import Fraction

import numpy as np

import indep_ref as ind

FULL_SCALE = 32767.0
ENV_N = 512                                    # samples of start-up envelope; the amplitude is settled behind them
A_INF = math.sqrt(0.95)                        # fixed point of a' = a (1.95 - a^2)
ANCHOR = 4096                                  # exact phase every ANCHOR samples of the absolute grid
TILE = 512                                     # the kernel's tile (dc_make_plan rounds the warm-up length to it)

# Parity tolerance relative to the rms of the reference output of a case: K = 4 x the largest
# max|dc_reference_fp32 - dc_reference| / rms(dc_reference) over all 164 plans on full-scale white input
# (tests/test_downconvert_ref_host.py measures it, prints it and asserts floor <= K / 4).
# Measured: 5.85e-7 at plan (11,11,15,23,51); four times that, rounded up to two digits.
K = 2.4e-6

_HDR = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "csdr_hb_taps.h")).read()
HB_LENS = [int(v) for v in re.search(r"csdr_hb_len\[[^\]]*\]\s*=\s*\{([^}]*)\}", _HDR).group(1).split(",") if v.strip()]
HB_EVEN = {L: [float(v) for v in re.search(r"/\* HB%d \*/ \{([^}]*)\}" % L, _HDR).group(1).split(",") if v.strip()]
           for L in HB_LENS}
KINDS = [3] + HB_LENS                          # the twelve stage kinds

_env = None


def envelope():
    """a_n, n < 512: downconvert.cpp's stabilising recurrence, through indep_ref.nco_mix at 0 Hz"""
    global _env
    if _env is None:
        _env = ind.nco_mix(np.ones(ENV_N), 0.0, 1.0).real.copy()
    return _env


def stage_taps(kind):
    """fp64 tap vector of a stage kind (the CIC-3 as the 4-tap FIR DecimateBy2 expects)"""
    return np.array([1.0, 3.0, 3.0, 1.0]) / 8.0 if kind == 3 else ind.halfband_taps(HB_EVEN[kind], kind)


def n_pairs(kind):
    return 2 if kind == 3 else (kind + 1) // 4


def hist_of(kind):
    return 2 if kind == 3 else kind - 1


def warmup_len(plan):
    """W of dc_host.hpp's dc_make_plan: sum_s hist_s 2^s rounded up to whole tiles (0 without stages)"""
    need = sum(hist_of(k) << s for s, k in enumerate(plan))
    unit = max(TILE, 1 << len(plan))
    return (need + unit - 1) // unit * unit if plan else 0


def mutate_pair(kind, q):
    """the stage's taps with tap pair q (taps 2q and L-1-2q; for the CIC 0/3 and 1/2) set to zero"""
    h = stage_taps(kind).copy()
    if kind == 3:
        h[[q, 3 - q]] = 0.0
    else:
        h[[2 * q, kind - 1 - 2 * q]] = 0.0
    return h


def mutate_centre(kind):
    """the centre tap moved by one sample; the CIC-3 has none: its two pair coefficients change places instead"""
    h = stage_taps(kind).copy()
    if kind == 3:
        return h[[1, 0, 3, 2]]
    c = (kind - 1) // 2
    h[c] = 0.0
    h[c + 1] += 0.5                               # (an even tap's place: the centre's weight lands on top of it)
    return h


def _turns(freq, rate):
    return Fraction(freq) / Fraction(rate)


class DcRef:
    """A streaming CDownConvert in fp64: run() takes calls of any length (multiples of 2^stages), set_frequency()
    retunes phase-continuously as SetFrequency does (the phasor stays, the increment changes).
    taps = {stage index: tap vector} replaces a stage's taps (the mutations of the tap-pair condition)."""

    def __init__(self, plan, freq, rate, first_sample=0, taps=None):
        self.plan, self.rate = tuple(plan), rate
        self.age = int(first_sample)
        self.turns = _turns(freq, rate)
        self.phase = (self.turns * self.age) % 1          # turns accumulated over the samples before `age`
        taps = taps or {}
        self.stages = [ind.DecimateBy2(taps.get(s, stage_taps(k))) for s, k in enumerate(self.plan)]

    def set_frequency(self, freq):
        self.turns = _turns(freq, self.rate)

    def mix(self, x):
        x = np.asarray(x, dtype=np.complex128)
        n = len(x)
        idx = self.age + np.arange(n, dtype=np.int64)
        ph = np.empty(n)
        # turns = hi + lo, hi on a 2^-32 grid: k * hi is exact for k < 4096 and reduced mod 1 before anything rounds
        hi = round(float(self.turns) * 2.0 ** 32) / 2.0 ** 32
        lo = float(self.turns - Fraction(hi))
        a0 = self.age - self.age % ANCHOR
        for anchor in range(a0, self.age + n, ANCHOR):
            b, e = max(anchor, self.age) - self.age, min(anchor + ANCHOR, self.age + n) - self.age
            # phase of absolute sample m: phase + (m - age + 1) turns; exact at the anchor, a float product behind it
            base = float((self.phase + (anchor - self.age + 1) * self.turns) % 1)
            k = (idx[b:e] - anchor).astype(np.float64)
            ph[b:e] = base + (k * hi) % 1.0 + k * lo
        amp = np.full(n, A_INF)
        early = idx < ENV_N
        amp[early] = envelope()[idx[early]]
        self.phase = (self.phase + n * self.turns) % 1
        self.age += n
        return x * amp * np.exp(2j * math.pi * ph)

    def run(self, x, from_stage=0):
        """x through the mixer and the cascade; from_stage = s > 0: x is stage s's input (already mixed)"""
        assert len(x) % (1 << (len(self.plan) - from_stage)) == 0
        y = self.mix(x) if from_stage == 0 else np.asarray(x, dtype=np.complex128)
        for st in self.stages[from_stage:]:
            y = st.run(y)
        return y


def dc_reference(plan, freq, rate, x, first_sample=0, calls=None, taps=None):
    """fp64 output of the cascade `plan` behind an NCO at `freq` for the input x whose first sample is sample
    `first_sample` of the stream (stage histories zero in front of it); calls = call lengths to cut x into (the
    result does not depend on them: test_downconvert_ref_host.py)"""
    r = DcRef(plan, freq, rate, first_sample, taps)
    if calls is None:
        return r.run(x)
    assert sum(calls) == len(x)
    out, pos = [], 0
    for n in calls:
        out.append(r.run(x[pos:pos + n])); pos += n
    return np.concatenate(out)


def stage_inputs(plan, freq, rate, x):
    """[input of stage 0 (the mixed stream), input of stage 1, ..., output]: lets a mutation of stage s be evaluated
    from stage s on (the cascade is feed-forward) instead of from the raw input every time"""
    r = DcRef(plan, freq, rate)
    ys = [r.mix(x)]
    for st in r.stages:
        ys.append(st.run(ys[-1]))
    return ys


def _stage_fp32(kind, x):
    """one decimate-by-2 stage in fp32 on a whole stream (zero history): centre product first, then acc + (a + b) c
    pair by pair in tap order, every operation rounded on its own"""
    xe = np.concatenate([np.zeros(hist_of(kind), dtype=np.complex64), x])
    nout = len(x) // 2
    tap = lambda k: xe[k:k + 2 * nout:2]                                   # xe[2j + k], j < nout
    if kind == 3:
        acc = (tap(1) + tap(2)) * np.float32(0.375)
        return acc + (tap(0) + tap(3)) * np.float32(0.125)
    acc = tap((kind - 1) // 2) * np.float32(0.5)
    for q in range(n_pairs(kind)):
        acc = acc + (tap(2 * q) + tap(kind - 1 - 2 * q)) * np.float32(HB_EVEN[kind][q])
    return acc


def dc_reference_fp32(plan, freq, rate, x, first_sample=0):
    """The formula of dc_reference evaluated in fp32: the phasor a_n e^{j phi_n} (phase exact) rounded to complex64,
    the mix a complex64 product, every stage as _stage_fp32.  One call, zero histories."""
    r = DcRef((), freq, rate, first_sample)
    phasor = r.mix(np.ones(len(x))).astype(np.complex64)
    x = np.asarray(x).astype(np.complex64)
    # (the four products and two sums written out on the real arrays: numpy rounds each ufunc on its own, while its
    # complex64 multiply may or may not fuse depending on the CPU it runs on)
    y = np.empty(len(x), dtype=np.complex64)
    y.real = x.real * phasor.real - x.imag * phasor.imag
    y.imag = x.real * phasor.imag + x.imag * phasor.real
    for k in plan:
        y = _stage_fp32(k, y)
        assert y.dtype == np.complex64
    return y


def rms(y):
    y = np.asarray(y)
    return float(np.sqrt(np.mean(y.real ** 2 + y.imag ** 2)))


def tolerance(ref):
    return K * rms(ref)


# ---------------------------------------------------------------------------------------------------------------------
# The parity case of a plan: the SAME input and call lengths on the CPU (floor, tap-pair condition) and on the GPU.
def parity_calls(plan):
    """three calls: whole tiles, a ragged middle call of 2048 + 3 * 2^ns, whole tiles.  The outer calls grow with the
    decimation so that the last stage still gives a few hundred outputs (the tap-pair condition needs the quietest
    tap of the LAST stage to show)."""
    u = 1 << len(plan)
    whole = max(8192, 128 * u)
    return [whole, 2048 + 3 * u, whole // 2]


PARITY_TURNS = 0.0703125 + 2.0 ** -20          # NCO of the parity cases, turns per sample (non-zero, not a tile period)


def plan_seed(plan):
    return int.from_bytes(bytes(plan), "little") % (2 ** 63) + 12345 if plan else 12345


def white(seed, n):
    """seeded full-scale white I/Q, uniform in +-32767 on both rails, as the fp32 values every consumer is given"""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = rng.uniform(-FULL_SCALE, FULL_SCALE, size=(n, 2)).astype(np.float32)
    return (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)


def parity_input(plan):
    return white(plan_seed(plan), sum(parity_calls(plan)))


def parity_freq(rate):
    return -PARITY_TURNS * rate


# ---------------------------------------------------------------------------------------------------------------------
# Impulse cases: one stage, NCO at 0 Hz, full-scale impulses behind the envelope -- the output IS the tap vector.
IMPULSE_AT = (1560, 1701)                      # one even, one odd input index; > 512, > 51 apart, inside tile 3
IMPULSE_VALUE = FULL_SCALE - 1j * FULL_SCALE


def impulse_input(n):
    x = np.zeros(n, dtype=np.complex64)
    x[list(IMPULSE_AT)] = IMPULSE_VALUE
    return x


def impulse_expected(kind, n):
    """y[j] = sum_m v a_inf h[m + hist - 2j] written out directly (no filter routine): exact zeros where no tap lands"""
    h, hist = stage_taps(kind), hist_of(kind)
    y = np.zeros(n // 2, dtype=np.complex128)
    for m in IMPULSE_AT:
        for j in range(n // 2):
            k = m + hist - 2 * j
            if 0 <= k < len(h):
                y[j] += IMPULSE_VALUE * A_INF * h[k]
    return y
